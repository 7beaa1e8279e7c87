"""The video-stream loop of tests/stream_oracle.py::oracle_stream restated one frame at a time with the tracker as a parameter, so
that the seeded reference (tests/lk_seed_reference.py) can stand where the loop calls io.lk_pyr.  As far as the tracks go this is
also the loop of oracle_node_fused: under OFK_KEEP_STATUS both keep the points with status 1 and re-detect alike.  With
`plain_lk` it must equal oracle_stream (tests/test_lk_seed_reference.py checks that on the CPU).  Test infrastructure only."""
import numpy as np

from oracle import image_oracle as io, estimation_oracle as eo
from stream_oracle import disc_mask


def plain_lk(cfg):
    return lambda g_prev, g, old: io.lk_pyr(g_prev, g, old, cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr)


class StreamLoop:
    """begin = goodFeaturesToTrack on the first frame; step(frame, sensors_row, lk) = node:131-175 with lk(g_prev, g, old) ->
    (next, status, err) as the tracker.  step returns (v_obs or None, tracks after the step, n_old, n_tracked)."""

    def __init__(self, first_frame, cfg, min_feat, radius):
        self.cfg, self.min_feat, self.radius = cfg, min_feat, radius
        self.h, self.w = first_frame.shape[:2]
        self.g_prev = io.gray_bgr8(first_frame)
        self.tracks = io.good_features(self.g_prev, cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size).reshape(-1, 2)

    def step(self, frame, sr, lk, normal=None, omega=None):
        cfg = self.cfg
        g = io.gray_bgr8(frame)
        old = self.tracks; n_old = len(old)
        if n_old:
            new, st, _ = lk(self.g_prev, g, old)
            new = new.reshape(-1, 2); ok = st.ravel() == 1
        else:
            new = np.zeros((0, 2), np.float32); ok = np.zeros(0, bool)
        x = (new[ok].astype(np.float64) - [sr[20], sr[21]]) * sr[19]; u = (new[ok].astype(np.float64) - old[ok]) * sr[19]
        nrm = sr[1:4] if normal is None else normal
        om = sr[4:7] if omega is None else omega
        v = eo.solve_lgs_node(x, u, sr[0], nrm, om)[0] if len(x) >= 3 else None
        tracked = new[ok]
        if n_old <= self.min_feat and cfg.max_corners - n_old > 0:
            mask = disc_mask(self.h, self.w, old, self.radius)
            newf = io.good_features(self.g_prev, cfg.max_corners - n_old, cfg.quality, cfg.min_distance, cfg.block_size, mask=mask).reshape(-1, 2)
            self.tracks = np.concatenate([tracked, newf])[:cfg.max_corners]
        else:
            self.tracks = tracked
        self.g_prev = g
        return v, self.tracks.copy(), n_old, int(ok.sum())


def run(frames, cfg, sensors, min_feat, radius, lk):
    """oracle_stream's return value: (first tracks, [(v, tracks, n_old, n_tracked) per step])."""
    loop = StreamLoop(frames[0], cfg, min_feat, radius)
    first = loop.tracks.copy()
    return first, [loop.step(frames[t], sensors, lk) for t in range(1, len(frames))]
