"""GPU parity of ofk_pairs_run at the batch sizes the benchmark runs and on both sides of every batch-dependent launch choice.

The launchers pick kernels and launch geometry by the (per-slice) batch: response strip rows (k_corners.hip ofk_stream_geometry),
k_select_greedy<1024> or <256> (ofk_launch_select), k_pairs_solve or k_pairs_solve_wg (ofk_launch_pairs_solve), the XCD-aware
block remap of LK and the pyramid kernels (gridDim.y % 8 == 0), the pyramid chunk counts.  Every pair is compared with the CPU
oracle chain (tests/batch_oracle.py) and its records with a run of the pair alone, bit for bit."""
import ast
import contextlib
import ctypes
import os

import numpy as np
import pytest

from batch_oracle import assert_pair_matches, assert_records_identical, oracle_many
from oracle import image_oracle as io
from test_gpu_response_f32 import TWO24, max_window_sum

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH_TRUTH = dict(v=(0.002, -0.0015, 0.001), omega=(0.002, -0.001, 0.003), d=1.0)      # bench.py main()
BENCH_SEED = 2000                                                                     # bench.py main(), rank 0


def bench_configs():
    """bench.py's CONFIGS, read from its source (the assignment node: literals and dict(...) calls only, evaluated without
    builtins), so that these tests follow the benchmark without importing it."""
    with open(os.path.join(ROOT, "bench.py")) as f:
        tree = ast.parse(f.read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "CONFIGS" for t in node.targets):
            return eval(compile(ast.Expression(node.value), "bench.py", "eval"), {"__builtins__": {}, "dict": dict})
    raise AssertionError("bench.py has no CONFIGS assignment")


def bench_cfg(C):
    from of_amd.pipeline import PipelineConfig
    return PipelineConfig(max_corners=C["corners"], quality=0.01, min_distance=10, block_size=7, win=15, max_level=C["levels"],
                          max_count=20, eps=0.03)


def bench_frames(C):
    """The benchmark's frames and sensors, built as bench.py main() builds them."""
    import of_amd.ofk as ofk
    from of_amd import synth
    prev, nxt, base = synth.make_batch(C["batch"], C["h"], C["w"], seed=BENCH_SEED, distinct=4, **BENCH_TRUTH)
    p0 = base[0]
    sensors = ofk.make_sensors(C["batch"], d=p0["d"], normal=p0["n"], omega=p0["omega"], scaling=p0["scaling"], cx=p0["cx"], cy=p0["cy"])
    return prev, nxt, sensors


# ---------------------------------------------------------------------------------------------------- the launchers' choices
def sel_tgt(max_corners):
    """k_corners.hip sel_tgt: keys per selection round."""
    t = 512
    while t < 2 * max_corners and t < 4096:
        t <<= 1
    return t


def strip_rows(h, nb):
    """k_corners.hip ofk_stream_geometry: response strip rows for a slice of nb images (no tuning knob set)."""
    if nb >= 64:
        k = (h + 269) // 270
        return (h + k - 1) // k
    return 128 if nb >= 16 else 32


def library_strip_rows(h, w, block, nb):
    import of_amd.ofk as ofk
    fn = getattr(ofk.load_library(), "_Z19ofk_stream_geometryiiiiPiS_S_")
    fn.restype = None
    rows, nseg, cap = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    fn(h, w, block, nb, ctypes.byref(rows), ctypes.byref(nseg), ctypes.byref(cap))
    return rows.value


def launch_sides(h, B, streams, max_corners):
    """What the launchers choose for each slice of a B-pair batch cut into `streams` slices."""
    S = min(streams, B)
    sides = []
    for k in range(S):
        nb = B * (k + 1) // S - B * k // S
        tgt = sel_tgt(max_corners)
        sides.append(dict(nb=nb, rows=strip_rows(h, nb), tgt=tgt, greedy=1024 if nb <= 64 and tgt >= 2048 else 256,
                          solve="wave" if nb >= 128 else "wg", lk_remap=nb % 8 == 0, pyr_remap=(2 * nb) % 8 == 0))
    return sides


@contextlib.contextmanager
def flow_pipeline(w, h, B, cfg, streams=1):
    """A FlowPipeline that is closed (its device buffers freed) even when an assertion fails inside."""
    from of_amd.pipeline import FlowPipeline
    pipe = FlowPipeline(w, h, B, cfg, streams=streams)
    try:
        yield pipe
    finally:
        pipe.close()


def run_alone(pipe, prev, nxt, sensors, params, idx):
    """Records of each pair in idx from a batch of one -> {pair: records row}."""
    pipe.ctx.set_streams(1)
    rec = {}
    for b in idx:
        pipe.ctx.pairs_upload(prev[b:b + 1], nxt[b:b + 1])
        pipe.ctx.pairs_set_sensors(sensors[b:b + 1])
        pipe.ctx.pairs_run(params)
        rec[b] = pipe.ctx.pairs_download(points=False)["records"][0].copy()
    return rec


def noise(shape, seed):
    """Full-contrast 0 / 255 noise: its 7 x 7 windows hold Sxx + Syy above 2^24."""
    return (np.random.default_rng(seed).integers(0, 2, shape) * 255).astype(np.uint8)


def put_gray(frames, b, region, patch):
    """Writes a gray patch into both frames of pair b (equal B, G, R: the gray conversion returns the patch itself)."""
    for f in frames:
        f[b][region] = patch[..., None]


def plateau_patch(bs, seed, pw=300):
    """A 0/255 tile whose period is the box size (test_gpu_response_f32: plateau rows of identical responses)."""
    rng = np.random.default_rng(seed)
    tile = (rng.integers(0, 2, (bs, bs)) * 255).astype(np.uint8)
    ph = 6 + 2 * (bs // 2 + 1) + 1
    return np.tile(tile, (ph // bs + 1, pw // bs + 1))[:ph, :pw]


# ---------------------------------------------------------------------------------------------------- 1. threshold sweep
SWEEP_H, SWEEP_W = 272, 448                    # multiple of 16 x 8: the three-level pyramid kernel; 136-row strips from B = 64
SWEEP_B = (1, 7, 8, 15, 16, 17, 63, 64, 65, 127, 128, 129, 136)
SWEEP_STREAMS2 = (130, 136)
NOISE_PAIRS = (5, 70, 131)                     # full-contrast noise in rows 100-125: a 136-row strip restarts ~100 rows in
PLATEAU_PAIRS = (9, 66, 133)                   # plateau rows of tied responses


def sweep_sets():
    from of_amd.pipeline import PipelineConfig
    return {
        "mc500": PipelineConfig(max_corners=500, quality=0.01, min_distance=10, block_size=7),       # tgtA 1024
        "mc600": PipelineConfig(max_corners=600, quality=0.005, min_distance=6, block_size=7),       # tgtA 2048
        "mc2000": PipelineConfig(max_corners=2000, quality=0.001, min_distance=3, block_size=7),     # tgtA 4096
        "multiround": PipelineConfig(max_corners=700, quality=0.001, min_distance=12, block_size=7),  # tgtA 2048, > 1 greedy round
    }


@pytest.fixture(scope="module")
def sweep_pool(pkg):
    import of_amd.ofk as ofk
    from of_amd import synth
    n = max(SWEEP_B + SWEEP_STREAMS2)
    prev, nxt, base = synth.make_batch(n, SWEEP_H, SWEEP_W, seed=4100, distinct=34, v=(0.003, -0.002, 0.0015),
                                       omega=(0.002, -0.001, 0.003), d=1.0)
    for b in NOISE_PAIRS:
        put_gray((prev, nxt), b, (slice(100, 126), slice(40, 400)), noise((26, 360), b))
    for b in PLATEAU_PAIRS:
        p = plateau_patch(7, b)
        put_gray((prev, nxt), b, (slice(150, 150 + p.shape[0]), slice(80, 80 + p.shape[1])), p)
    sensors = np.concatenate([ofk.make_sensors(1, d=base[b % 34]["d"], normal=base[b % 34]["n"], omega=base[b % 34]["omega"],
                                               scaling=base[b % 34]["scaling"], cx=base[b % 34]["cx"], cy=base[b % 34]["cy"]) for b in range(n)])
    return prev, nxt, sensors


@pytest.mark.parametrize("name", ["mc500", "mc600", "mc2000", "multiround"])
def test_launch_threshold_sweep(pkg, ofk, sweep_pool, name):
    prev, nxt, sensors = sweep_pool
    cfg = sweep_sets()[name]
    n = len(prev)
    for b in NOISE_PAIRS:                                       # the band crosses 2^24 (integer rows), the rest of the frame does not
        g = io.gray_bgr8(prev[b])
        assert max_window_sum(g[90:136], 7) >= TWO24 and max_window_sum(g[:80], 7) < TWO24 - 256
    if name == "multiround":                                    # the last accepted corner lies past the first round's keys
        for b in range(0, n, 9):
            g = io.gray_bgr8(prev[b])
            ranked = io.select_corners(io.mineig(g, cfg.block_size), 0, cfg.quality, 0)[0].reshape(-1, 2)
            last = io.good_features(g, cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size).reshape(-1, 2)[-1]
            rank = int(np.flatnonzero((ranked == last).all(1))[0])
            assert rank >= sel_tgt(cfg.max_corners), (b, rank)
    ref = oracle_many(prev, nxt, cfg, sensors, range(n))
    params = cfg.to_params()
    seen = []
    with flow_pipeline(SWEEP_W, SWEEP_H, n, cfg) as pipe:                # one context, sized for the largest batch
        alone = run_alone(pipe, prev, nxt, sensors, params, range(n))
        for B, streams in [(B, 1) for B in SWEEP_B] + [(B, 2) for B in SWEEP_STREAMS2]:
            sides = launch_sides(SWEEP_H, B, streams, cfg.max_corners)
            for s in sides:
                assert library_strip_rows(SWEEP_H, SWEEP_W, cfg.block_size, s["nb"]) == s["rows"], s
                seen.append(dict(s, streams=streams))
            pipe.ctx.set_streams(streams)
            pipe.ctx.pairs_upload(prev[:B], nxt[:B])
            pipe.ctx.pairs_set_sensors(sensors[:B])
            pipe.ctx.pairs_run(params)
            out = pipe.ctx.pairs_download()
            for b in range(B):
                assert_pair_matches(out, b, ref[b], f"B={B} streams={streams} {name}")
                assert_records_identical(out["records"][b], alone[b], f"pair {b} B={B} streams={streams} vs B=1")
    # both sides of every threshold ran
    assert {s["rows"] for s in seen} == {32, 128, 136}
    assert {s["solve"] for s in seen} == {"wave", "wg"}
    assert {s["lk_remap"] for s in seen} == {True, False} and {s["pyr_remap"] for s in seen} == {True, False}
    assert {s["greedy"] for s in seen} == ({1024, 256} if sel_tgt(cfg.max_corners) >= 2048 else {256})
    # two slices: B >= 128 overall, but each slice launches with 64 < nb < 128 (136-row strips, k_select_greedy<256>, k_pairs_solve_wg)
    assert all(64 < s["nb"] < 128 and s["rows"] == 136 and s["greedy"] == 256 and s["solve"] == "wg" for s in seen if s["streams"] == 2)


# ---------------------------------------------------------------------------------------------------- 2. c1 as benchmarked
def test_c1_as_benchmarked(pkg, ofk):
    C = bench_configs()["c1"]
    assert not C["ekf"]
    cfg = bench_cfg(C)
    B = C["batch"]
    frames = bench_frames(C)
    try:
        with flow_pipeline(C["w"], C["h"], B, cfg, C["streams"]) as pipe:
            prev, nxt, sensors = frames
            pipe.upload(prev, nxt, sensors)
            for _ in range(3 + 5):                               # bench.py run_steps: warm-up, then timed steps, back to back
                pipe.run_async()
            out = pipe.ctx.pairs_download()
            plain = pipe.run()
        ref = oracle_many(prev, nxt, cfg, sensors, range(B))
    finally:
        del frames                                               # 6.4 GB of frames: not kept alive by a failure's traceback
        prev = nxt = None
    for b in range(B):
        assert_pair_matches(out, b, ref[b], "c1")
    assert_records_identical(plain["records"], out["records"], "c1 run() vs run_async x 8")
    assert np.array_equal(plain["counts"], out["counts"])
    for b in range(B):
        n = int(out["counts"][b])
        for k in ("prev_pts", "next_pts", "err"):
            assert np.array_equal(plain[k][b, :n].view(np.uint32), out[k][b, :n].view(np.uint32)), (b, k)
        assert np.array_equal(plain["status"][b, :n], out["status"][b, :n]), b


# ---------------------------------------------------------------------------------------------------- 3. mixed content, 1080p
def test_mixed_content_1080p_batch_136(pkg, ofk):
    from of_amd import synth
    C = bench_configs()["c1"]
    cfg = bench_cfg(C)
    h, w, B = C["h"], C["w"], 136
    assert strip_rows(h, B) == 270 and B % 8 == 0 and B > 128
    prev, nxt, base = synth.make_batch(B, h, w, seed=BENCH_SEED, distinct=4, **BENCH_TRUTH)
    ref_bgr = np.load(os.path.join(ROOT, "tests", "golden", "reference_frame.npz"))["frame_bgr"]
    real = np.tile(ref_bgr, (h // ref_bgr.shape[0] + 1, w // ref_bgr.shape[1] + 1, 1))[:h, :w]
    rng = np.random.default_rng(77)
    dots = np.full((h, w, 3), 60, np.uint8)
    for y, x in zip(rng.integers(40, h - 40, 8), rng.integers(40, w - 40, 8)):
        dots[y - 1:y + 2, x - 1:x + 2] = 230
    kinds = ("texture", "noise_band", "plateau", "real", "flat", "dots")
    for b in range(B):
        kind = kinds[b % len(kinds)]
        if kind == "noise_band":                                 # crosses 2^24 first 230 rows into the 270-row strip at 270
            put_gray((prev, nxt), b, (slice(500, 531), slice(1000, 1300)), noise((31, 300), b))
        elif kind == "plateau":
            bg = rng.integers(100, 112, (h, w)).astype(np.uint8)
            p = plateau_patch(7, b)
            bg[40:40 + p.shape[0], 100:100 + p.shape[1]] = p
            prev[b] = nxt[b] = bg[..., None]
        elif kind == "real":
            prev[b] = real; nxt[b] = np.roll(real, (1, 2), axis=(0, 1))
        elif kind == "flat":
            prev[b] = nxt[b] = 128
        elif kind == "dots":
            prev[b] = dots; nxt[b] = np.roll(dots, (1, -1), axis=(0, 1))
    g = io.gray_bgr8(prev[1])
    assert max_window_sum(g[480:540], 7) >= TWO24 and max_window_sum(g[270:490], 7) < TWO24 - 256
    p0 = base[0]
    sensors = ofk.make_sensors(B, d=p0["d"], normal=p0["n"], omega=p0["omega"], scaling=p0["scaling"], cx=p0["cx"], cy=p0["cy"])
    with flow_pipeline(w, h, B, cfg) as pipe:
        pipe.upload(prev, nxt, sensors)
        out = pipe.run()
        alone = run_alone(pipe, prev, nxt, sensors, cfg.to_params(), range(B))
    ref = oracle_many(prev, nxt, cfg, sensors, range(B))
    counts = {k: [] for k in kinds}
    for b in range(B):
        assert_pair_matches(out, b, ref[b], kinds[b % len(kinds)])
        counts[kinds[b % len(kinds)]].append(int(out["counts"][b]))
    assert max(counts["flat"]) == 0 and min(counts["texture"]) == cfg.max_corners
    assert 3 <= min(counts["dots"]) and max(counts["dots"]) < 50
    for b in range(B):
        assert_records_identical(out["records"][b], alone[b], f"pair {b} ({kinds[b % len(kinds)]}) B={B} vs B=1")


# ---------------------------------------------------------------------------------------------------- 4. c4 as benchmarked
def test_c4_as_benchmarked(pkg, ofk):
    """The benchmark's k_select_greedy<256> with tgtA 4096 (the sweep reaches the same path on small frames).  All 256 pairs: the
    context holds ~44 GB of device memory, the frames ~13 GB of host memory; both are freed before the test returns."""
    C = bench_configs()["c4"]
    cfg = bench_cfg(C)
    B = C["batch"]
    sides = launch_sides(C["h"], B, C["streams"], cfg.max_corners)
    assert [s["greedy"] for s in sides] == [256] and sides[0]["tgt"] == 4096 and sides[0]["rows"] == 270
    frames = bench_frames(C)
    try:
        with flow_pipeline(C["w"], C["h"], B, cfg, C["streams"]) as pipe:
            prev, nxt, sensors = frames
            pipe.upload(prev, nxt, sensors)
            out = pipe.run()
            alone = run_alone(pipe, prev, nxt, sensors, cfg.to_params(), [0])
        ref = oracle_many(prev, nxt, cfg, sensors, range(B))
    finally:
        del frames                                               # ~13 GB
        prev = nxt = None
    for b in range(B):
        assert_pair_matches(out, b, ref[b], "c4")
    assert_records_identical(out["records"][0], alone[0], "c4 pair 0 vs B=1")


# ---------------------------------------------------------------------------------------------------- 5. c2 as benchmarked
def test_c2_as_benchmarked_with_filter(pkg, ofk):
    from oracle import estimation_oracle as eo
    from of_amd.pipeline import FilterModel
    C = bench_configs()["c2"]
    assert C["ekf"] and C["streams"] == 2
    cfg = bench_cfg(C)
    B, K = C["batch"], 3 + 5
    prev, nxt, sensors = bench_frames(C)
    m = FilterModel.ekf6()
    with flow_pipeline(C["w"], C["h"], B, cfg, C["streams"]) as pipe:
        pipe.upload(prev, nxt, sensors)
        pipe.ctx.filter_configure(m, B)
        for _ in range(K):                                       # bench.py run_steps with ekf: the filter update behind every step
            pipe.run_async()
            pipe.ctx.pairs_filter_step(B)
        out = pipe.ctx.pairs_download()
        x, P = pipe.ctx.filter_state(B)
    ref = oracle_many(prev, nxt, cfg, sensors, range(B))
    for b in range(B):
        assert_pair_matches(out, b, ref[b], "c2")
    v_obs = out["records"][:, :3]
    for b in range(B):
        xr, Pr = np.array(m.x0, np.float64), np.array(m.P0, np.float64)
        for _ in range(K):
            xr, Pr = eo.kf_predict(xr, Pr, m.F, m.Q)
            xr, Pr = eo.kf_correct(xr, Pr, m.H, m.R, -v_obs[b])
        np.testing.assert_allclose(x[b], xr, rtol=1e-11, atol=1e-18, err_msg=str(b))
        np.testing.assert_allclose(P[b], Pr, rtol=1e-10, atol=1e-14, err_msg=str(b))
