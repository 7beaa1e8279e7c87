"""The greedy corner selection with a per-cell cap (include/ofk.h: ofk_corner_grid) restated in numpy on the CPU oracle's response
map: the reference the corner-grid tests compare the device against, and a NodeLoop whose detections run through it.  With the grid
off it is goodFeaturesToTrack's selection (oracle.image_oracle.select_corners, tested).  Test infrastructure only."""
import numpy as np

from oracle import image_oracle as io
from stream_oracle import NodeLoop

MAX_CELLS = 2048                                                 # OFK_GRID_MAX_CELLS
OFF = (0, 0, 0)                                                  # (cell, cap, max_rank)


def candidates(eig, quality, mask=None):
    """Linear indices of the candidates in rank order: inside the mask, > f32(f64(max over the mask) * quality), a 3x3 local maximum
    of the interior; value descending, then index descending."""
    eig = np.ascontiguousarray(eig, np.float32)
    h, w = eig.shape
    live = np.ones((h, w), bool) if mask is None else np.asarray(mask) != 0
    if not live.any():
        return np.zeros(0, np.int64)
    maxv = eig[live].max()
    if not maxv > 0:
        return np.zeros(0, np.int64)
    thr = np.float32(np.float64(maxv) * quality)
    c = eig[1:-1, 1:-1]
    ok = (c > thr) & live[1:-1, 1:-1]
    for dy in range(3):
        for dx in range(3):
            ok &= ~(eig[dy:dy + h - 2, dx:dx + w - 2] > c)
    ys, xs = np.nonzero(ok)
    idx = (ys + 1).astype(np.int64) * w + xs + 1
    order = np.lexsort((-idx, -eig.ravel()[idx].astype(np.float64)))
    return idx[order]


def occupancy(h, w, cell, occ_pts):
    """Corners per cell of the listed points: truncated position, points outside the image (or not a number) ignored."""
    gw, gh = -(-w // cell), -(-h // cell)
    occ = np.zeros(gw * gh, np.int64)
    for x, y in np.asarray(occ_pts if occ_pts is not None else [], np.float32).reshape(-1, 2):
        if np.isfinite(x) and np.isfinite(y) and 0 <= int(x) < w and 0 <= int(y) < h and x > -1 and y > -1:
            occ[(int(y) // cell) * gw + int(x) // cell] += 1
    return occ


def select(eig, max_corners, quality, min_distance, mask=None, grid=OFF, occ_pts=None):
    """-> (points [n,2] f32, (accepted, examined), ranks of the accepted candidates).  grid = (cell, cap, max_rank)."""
    cell, cap, max_rank = grid
    h, w = np.shape(eig)
    idx = candidates(eig, quality, mask)
    md = np.float32(min_distance); md2 = md * md
    if cell > 0:
        gw = -(-w // cell)
        assert gw * -(-h // cell) <= MAX_CELLS and cap >= 1 and max_rank >= 0
        occ = occupancy(h, w, cell, occ_pts)
    acc, ranks, examined = [], [], 0
    ax, ay = np.zeros(max(max_corners, 1), np.int64), np.zeros(max(max_corners, 1), np.int64)
    for r, i in enumerate(idx):
        if len(acc) >= max_corners or (cell > 0 and ((occ >= cap).all() or (max_rank and r >= max_rank))):
            break
        examined = r + 1
        x, y = int(i % w), int(i // w)
        if cell > 0:
            c = (y // cell) * gw + x // cell
            if occ[c] >= cap:
                continue
        n = len(acc)
        if md >= 1 and n and (np.float32((ax[:n] - x) ** 2 + (ay[:n] - y) ** 2) < md2).any():
            continue
        ax[n], ay[n] = x, y
        acc.append((x, y)); ranks.append(r)
        if cell > 0:
            occ[c] += 1
    return np.array(acc, np.float32).reshape(-1, 2), (len(acc), examined), np.array(ranks, np.int64)


def good_features(gray, max_corners, quality, min_distance, block, mask=None, grid=OFF, occ_pts=None):
    return select(io.mineig(gray, block), max_corners, quality, min_distance, mask, grid, occ_pts)


def grid_detect(cfg, grid, log=None):
    """stream_oracle.NodeLoop's detection plug through the grid.  log (a list) receives every call's (accepted, examined)."""
    def detect(gray, budget, mask, occ_pts):
        pts, stats, _ = good_features(gray, budget, cfg.quality, cfg.min_distance, cfg.block_size, mask=mask, grid=grid, occ_pts=occ_pts)
        if log is not None:
            log.append(stats)
        return pts
    return detect


class GridNodeLoop(NodeLoop):
    """NodeLoop whose first detection runs through the grid with empty cells and whose re-detection (append mode, node:160-172) runs
    through it behind the same disc mask with the old tracks as the occupancy list (stream_oracle.NodeLoop's detect=)."""

    def __init__(self, first_frame, cfg, min_feat, radius, grid, **kw):
        super().__init__(first_frame, cfg, min_feat, radius, detect=grid_detect(cfg, grid), **kw)
        self.grid = grid
