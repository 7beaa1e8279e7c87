"""Restatements of the launchers' routing rules for the LK window and corner block-size axes, the image patterns that drive the
kernels' integer sums to their limits, and the case generator of the randomised pipeline sweep (shared by
tests/test_gpu_param_ranges.py and tools/stress_parity.py).  Test infrastructure only: numpy and the CPU oracle, no GPU."""
import numpy as np

from oracle import image_oracle as io

LK_MAX_LEVELS = 9                      # ofk_internal.h OFK_MAX_LEVELS: levels 0 .. 8
LK_M = 8                               # k_lk.hip LK_M: margin of the staged next-frame region
INT32_MAX = 2 ** 31 - 1
LK_KERNELS = {"k_lk15q", "k_lk15", "k_lk<21>", "k_lk<31>"}
LK15_STAGING = {"prev_dword", "prev_byte", "next_dword", "next_byte"}


# ---------------------------------------------------------------------------------------------------- LK
def lk_level_sizes(h, w, win, max_level):
    """ofk_api.hip ofk_make_levels: [(h_l, w_l)] for l = 0 .. L; level l + 1 is ((h_l + 1) / 2, (w_l + 1) / 2) and exists while both
    sides stay above the window."""
    sizes = [(h, w)]
    while len(sizes) - 1 < max_level and len(sizes) < LK_MAX_LEVELS:
        nh, nw = (sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2
        if nw <= win or nh <= win:
            break
        sizes.append((nh, nw))
    return sizes


def cut_sizes(win):
    """Image sides n > win at which a level of the (n + 1) / 2 chain lands on win (that level is cut) or on win + 1 (it is kept),
    one or two halvings down: n in {2t - 1, 2t, 4t - 3, 4t} for t in {win, win + 1}."""
    return sorted({n for t in (win, win + 1) for n in (2 * t - 1, 2 * t, 4 * t - 3, 4 * t) if n > win})


def lk_kernel(h, w, win, max_level):
    """k_lk.hip ofk_launch_lk: the kernel that tracks a (h, w) pair (level offsets are 256-byte multiples, so only the sizes decide)."""
    sizes = lk_level_sizes(h, w, win, max_level)
    if win == 15 and all(lw % 4 == 0 and lw >= 40 and lh >= 32 for lh, lw in sizes):
        return "k_lk15q"
    if win <= 15:
        return "k_lk15"
    return "k_lk<21>" if win <= 21 else "k_lk<31>"


def lk15_staging(h, w, win, max_level, pts, margin=4):
    """The staging variants k_lk15 takes for points `pts` (N x 2): a subset of LK15_STAGING.  The previous-frame window of level l
    sits at the scaled point (exact); the first next-frame region of a level sits at the scaled point plus the flow found so far, so
    a point counts for the next-frame dword or byte path only where it is more than `margin` pixels inside that side of the test.
    The tests are k_lk15's: prev dwords when ipx >= 5, ipx + 27 <= lw, lw % 4 == 0; next dwords when win == 15, jx0 >= 4,
    jx0 + 40 <= lw, lw % 4 == 0."""
    half = np.float32((win - 1) / 2)
    seen = set()
    for l, (lh, lw) in enumerate(lk_level_sizes(h, w, win, max_level)):
        sc = np.float32(2.0 ** -l)
        for x, y in np.asarray(pts, np.float32).reshape(-1, 2):
            ipx, ipy = int(np.floor(x * sc - half)), int(np.floor(y * sc - half))
            if ipx < -win or ipx >= lw or ipy < -win or ipy >= lh:
                continue
            seen.add("prev_dword" if lw % 4 == 0 and ipx >= 5 and ipx + 27 <= lw else "prev_byte")
            jx0 = ipx - LK_M
            if win == 15 and lw % 4 == 0 and jx0 >= 4 + margin and jx0 + 40 + margin <= lw and margin <= ipy < lh - margin:
                seen.add("next_dword")
            elif win != 15 or lw % 4 != 0 or jx0 < 4 - margin or jx0 + 40 - margin > lw:
                seen.add("next_byte")
    return seen


def window_sums(gray, pts, win):
    """Level-0 normal-matrix sums sum(Ix^2), sum(Ix Iy), sum(Iy^2) (int64) of the windows of points at INTEGER positions: there the
    bilinear weights are (2^14, 0, 0, 0) and the window's Ix, Iy are the Scharr derivatives themselves (io.scharr; the window must lie
    inside the image)."""
    d = io.scharr(gray).astype(np.int64)
    half = (win - 1) // 2
    out = []
    for x, y in np.asarray(pts).reshape(-1, 2):
        x, y = int(x), int(y)
        wd = d[y - half:y + half + 1, x - half:x + half + 1]
        assert wd.shape[:2] == (win, win), (x, y, win)
        ix, iy = wd[..., 0], wd[..., 1]
        out.append(((ix * ix).sum(), (ix * iy).sum(), (iy * iy).sum()))
    return np.array(out, np.int64).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------- corners
def mineig_oh(bs):
    """k_corners.hip mineig_oh: response rows of one LDS-tile block."""
    return min(32, max(8, 33 - bs))


def pair_ok(w, bs):
    """k_corners.hip pair_ok (no tuning knob set)."""
    return bs in (3, 5, 7) and w % 4 == 0 and w >= 64


def corner_kernels(h, w, bs):
    """(kernel of ofk_mineig_response, candidate kernel of ofk_good_features) for a (h, w) image at block size bs."""
    resp = f"k_mineig<{bs},false>" if bs in (3, 7, 12) else "k_mineig<0,false>"
    if pair_ok(w, bs):
        cand = "k_mineig_pair"
    elif bs in (3, 5, 7, 12):
        cand = "k_mineig_stream"
    else:
        cand = "k_mineig<0,true>"
    return resp, cand


def tile_edge_shapes(bs):
    """Odd image sizes whose width and height straddle the LDS-tile blocks at block size bs: one column past / short of (at least
    two) multiples of the fused interior width 62 and of the map tile width 64, heights likewise for OH - 2 and OH rows."""
    oh = mineig_oh(bs)

    def straddle(period, delta):
        k = max(2, -(-(bs + 4 - delta) // period))
        return k * period + delta

    return [(straddle(oh - 2, 1), straddle(62, 1)), (straddle(oh, -1), straddle(64, -1)), (straddle(oh - 2, -1), straddle(64, 1)),
            (straddle(oh, 1), straddle(62, -1))]


# ---------------------------------------------------------------------------------------------------- images
def binary_noise(shape, seed):
    return (np.random.default_rng(seed).integers(0, 2, shape) * 255).astype(np.uint8)


def stripes(shape, axis=1, flip_rows=0):
    """Period-4 stripes (two lines at 0, two at 255): the central difference across them is +-255 everywhere, so Scharr |Ix| = 4080
    and Sobel |dx| = 1020.  axis=0 gives horizontal stripes.  flip_rows > 0 inverts every flip_rows-th row."""
    n = np.arange(shape[axis])
    line = (((n // 2) % 2) * 255).astype(np.uint8)
    img = np.broadcast_to(line[None, :] if axis == 1 else line[:, None], shape).copy()
    if flip_rows:
        img[::flip_rows] ^= 255
    return img


def diagonal(shape):
    """((x + y) / 2) mod 2 at full contrast: Ix and Iy both large and correlated (A12 close to A11)."""
    h, w = shape
    return (((np.add.outer(np.arange(h), np.arange(w)) // 2) & 1) * 255).astype(np.uint8)


def plaid(shape, seed=0):
    """Period-4 vertical stripes of amplitude 240 under faint noise (0..15): Sobel |dx| stays near 960 and dy is small but not zero,
    so Sxx stays near its limit while lambda_min is not zero (pure stripes give lambda_min = 0 whatever Sxx is) and the responses do
    not tie (a plateau of tied maxima overflows the streaming kernels' key segments by design: OFK_E_CAPACITY)."""
    noise = np.random.default_rng(seed).integers(0, 16, shape)
    return (stripes(shape, 1).astype(np.int32) * 240 // 255 + noise).astype(np.uint8)


def textured(h, w, seed):
    """synth.make_texture as uint8 (cut from a texture of at least 64 x 64 so that tiny frames look like crops of a larger one)."""
    from of_amd import synth
    t = np.clip(np.rint(synth.make_texture(max(h, 64), max(w, 64), seed)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(t[:h, :w])


def sobel_box_sums(gray, bs):
    """int64 restatement of the response's box sums Sxx, Sxy, Syy (Sobel products, REFLECT_101, window [p - bs/2, p - bs/2 + bs))."""
    g = gray.astype(np.int64)
    h, w = g.shape

    def r101(i, n):
        i = np.abs(i)
        return np.where(i >= n, 2 * (n - 1) - i, i)

    xs, ys = np.arange(w), np.arange(h)
    cx = g[:, r101(xs + 1, w)] - g[:, r101(xs - 1, w)]
    dx = cx[r101(ys - 1, h)] + 2 * cx + cx[r101(ys + 1, h)]
    cy = g[r101(ys + 1, h)] - g[r101(ys - 1, h)]
    dy = cy[:, r101(xs - 1, w)] + 2 * cy + cy[:, r101(xs + 1, w)]
    an = bs // 2

    def box(p):
        hs = sum(p[:, r101(xs - an + i, w)] for i in range(bs))
        return sum(hs[r101(ys - an + j, h)] for j in range(bs))

    return box(dx * dx), box(dx * dy), box(dy * dy)


# ---------------------------------------------------------------------------------------------------- randomised pipeline sweep
SWEEP_WIDTHS = (64, 68, 112, 116, 120, 124, 128, 232, 236, 240, 244, 348, 352, 464, 468, 496, 500, 504, 512, 640, 700, 992, 1000,
                322, 333, 479)                         # strip boundaries of the streaming kernels and odd widths


def sweep_cases(n_cases, seed, max_h=300):
    """Random FlowPipeline configurations: every odd LK window 3..31, block sizes 1..45 (the streaming kernels' 3/5/7/12 drawn more
    often), corner budgets, quality levels, pyramid depths, batches of 1-3 frame pairs with random motion.  Heights are at least
    block + 4 (what check_block accepts).  Deterministic in (n_cases, seed)."""
    from of_amd.pipeline import PipelineConfig
    rng = np.random.default_rng(seed)
    cases = []
    for case in range(n_cases):
        w = int(rng.choice(SWEEP_WIDTHS))
        bs = int(rng.choice([3, 5, 7, 12])) if rng.random() < 0.4 else int(rng.integers(1, 46))
        h = int(rng.integers(max(48, bs + 4), max_h))
        win = int(rng.choice(np.arange(3, 32, 2)))
        cfg = PipelineConfig(max_corners=int(rng.choice([10, 60, 200])), quality=float(rng.choice([0.01, 0.05, 0.2])),
                             min_distance=float(rng.choice([3, 7, 10])), block_size=bs, win=win, max_level=int(rng.integers(0, 4)),
                             max_count=int(rng.choice([10, 20])), eps=0.03)
        B = int(rng.integers(1, 4))
        motion = [dict(seed=9000 + 17 * case + b, v=tuple(rng.normal(0, 0.004, 3)), omega=tuple(rng.normal(0, 0.003, 3)))
                  for b in range(B)]
        cases.append(dict(case=case, h=h, w=w, B=B, cfg=cfg, motion=motion))
    return cases


def describe(c):
    cfg = c["cfg"]
    return (f"case {c['case']:3d}: {c['w']}x{c['h']} B={c['B']} bs={cfg.block_size} win={cfg.win} lvl={cfg.max_level} "
            f"corners<={cfg.max_corners} q={cfg.quality}")


def sweep_frames(c):
    """The frame pairs and sensor rows of a sweep case."""
    import of_amd.ofk as ofk
    from of_amd import synth
    pairs = [synth.render_pair(c["h"], c["w"], m["seed"], v=m["v"], omega=m["omega"], d=1.0) for m in c["motion"]]
    prev = np.stack([p["prev"] for p in pairs]); nxt = np.stack([p["next"] for p in pairs])
    sensors = np.concatenate([ofk.make_sensors(1, scaling=p["scaling"], cx=p["cx"], cy=p["cy"]) for p in pairs])
    return prev, nxt, sensors


def sweep_oracle(prev, nxt, cfg):
    """CPU oracle of each pair: [(corners (N, 2), next points (N, 2), status (N,), err (N,))]; raises ValueError where the oracle
    refuses the configuration."""
    out = []
    for b in range(len(prev)):
        g0, g1 = io.gray_bgr8(prev[b]), io.gray_bgr8(nxt[b])
        pts = io.good_features(g0, cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size)
        nx, st, er = io.lk_pyr(g0, g1, pts, cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr)
        out.append((pts.reshape(-1, 2), nx.reshape(-1, 2), st.ravel(), er.ravel()))
    return out


def sweep_mismatches(out, ref):
    """Pairs whose FlowPipeline outputs differ from the oracle's: corners, status, next points and err bit for bit."""
    bad = []
    for b, (pts, nx, st, er) in enumerate(ref):
        n = int(out["counts"][b])
        ok = n == len(pts) and np.array_equal(out["prev_pts"][b, :n].view(np.uint32), pts.view(np.uint32))
        ok = ok and np.array_equal(out["status"][b, :n], st)
        ok = ok and np.array_equal(out["next_pts"][b, :n].view(np.uint32), nx.view(np.uint32))
        ok = ok and np.array_equal(out["err"][b, :n].view(np.uint32), er.view(np.uint32))
        if not ok:
            bad.append(b)
    return bad


def run_sweep_case(c, ofk):
    """One sweep case through FlowPipeline and the oracle -> None when they agree (or both refuse), else a description."""
    from of_amd.pipeline import FlowPipeline
    prev, nxt, sensors = sweep_frames(c)
    try:
        ref = sweep_oracle(prev, nxt, c["cfg"])
    except ValueError as e:
        ref = e
    try:
        pipe = FlowPipeline(c["w"], c["h"], c["B"], c["cfg"])
        try:
            pipe.upload(prev, nxt, sensors)
            out = pipe.run()
        finally:
            pipe.close()
    except ofk.OfkError as e:
        return None if isinstance(ref, ValueError) else f"{describe(c)}: library refused: {e}"
    if isinstance(ref, ValueError):
        return f"{describe(c)}: the oracle refused ({ref}), the library ran"
    bad = sweep_mismatches(out, ref)
    return f"{describe(c)}: MISMATCH in pairs {bad}" if bad else None
