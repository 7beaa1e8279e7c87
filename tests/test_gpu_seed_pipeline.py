"""GPU: the LK seed setting (ofk_set_lk_seed) through ofk_pairs_run and the stream steps, against the test-side reference
(tests/lk_seed_reference.py) fed with the seeds ofk_predict_points returns for the downloaded points.

(a) ofk_pairs_run, OFK_SEED_MODEL / OFK_SEED_ROTATION: every pair of every batch is compared (the reference is compiled C).
(b) the fast-manoeuvre experiment end to end on the device, held to the conditions of tests/lk_seed_reference.py.
(c) FlowStream.step / step_fused (sensors and resident IMU state as the seed's source) against the restated stream loop.
(d) seed mode off after having been on: bit-identical to a context that never had it."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import image_oracle as io, estimation_oracle as eo
import lk_seed_reference as R  # noqa: E402  (tests/lk_seed_reference.py)
from stream_oracle import NodeLoop, imu_messages  # noqa: E402  (tests/stream_oracle.py)

pytestmark = pytest.mark.gpu

MOTION = dict(v=(0.012, -0.008, 0.002), omega=(0.004, -0.003, 0.03), d=1.0)      # flows of 10-20 px at 640 x 480
MAX_BATCH = {(480, 640): 256, (1080, 1920): 130}                                  # rendered once per size
_batches = {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def batch_frames(h, w, B):
    key = (h, w)
    if key not in _batches:
        from of_amd import synth
        _batches[key] = synth.make_batch(MAX_BATCH[key], h, w, seed=3100, distinct=4, margin=96, **MOTION)
    prev, nxt, base = _batches[key]
    return prev[:B], nxt[:B], base


def compare_pairs(ofk, ctx, out, prev, nxt, sensors, cfg, mode, gain, tag):
    """Every pair: LK outputs against the reference run on the downloaded points with the seeds ofk_predict_points returns."""
    B = len(prev)
    counts = out["counts"]
    seeds = ctx.predict_points(out["prev_pts"], counts, sensors, mode, gain)
    flags = R.USE_INITIAL_FLOW

    def one(b):
        n = int(counts[b])
        g0, g1 = io.gray_bgr8(prev[b]), io.gray_bgr8(nxt[b])
        ref_pts = io.good_features(g0, cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size).reshape(-1, 2)
        p = out["prev_pts"][b, :n]
        rn, rs, re = R.lk_pyr(g0, g1, p, cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr, seed=seeds[b, :n], flags=flags)
        return ref_pts, rn.reshape(-1, 2), rs.ravel(), re.ravel()

    with ThreadPoolExecutor(16) as ex:
        refs = list(ex.map(one, range(B)))
    moved = 0
    for b, (ref_pts, rn, rs, re) in enumerate(refs):
        n = int(counts[b]); t = (tag, "pair", b)
        assert n == len(ref_pts) and np.array_equal(bits(out["prev_pts"][b, :n]), bits(ref_pts)), t
        want_seed = R.predict(ref_pts, sensors[b], mode, gain)
        assert np.all(np.abs(seeds[b, :n].view(np.int32).astype(np.int64) - want_seed.view(np.int32)) <= 1), t
        assert np.array_equal(bits(out["next_pts"][b, :n]), bits(rn)), t
        assert np.array_equal(out["status"][b, :n], rs), t
        assert np.array_equal(bits(out["err"][b, :n]), bits(re)), t
        ok = rs == 1
        sr = sensors[b]
        x = (rn[ok].astype(np.float64) - [sr[20], sr[21]]) * sr[19]; u = (rn[ok].astype(np.float64) - ref_pts[ok]) * sr[19]
        rec = out["records"][b]
        assert rec[12] == n and rec[13] == int(ok.sum()), t
        if len(x) >= 3:
            v = eo.solve_lgs_node(x, u, sr[0], sr[1:4], sr[4:7])[0]
            np.testing.assert_allclose(rec[0:3], v, rtol=1e-10, atol=1e-13, err_msg=str(t))
        moved += int(np.sum(np.abs(seeds[b, :n] - ref_pts) > 2))
    assert moved > 0, tag                                         # the seeds are not the points: the run was seeded


# size, batch, corners, mode, max_level, slices, overlap.  The solve takes k_pairs_solve from 128 pairs per slice on, k_pairs_solve_wg below.
PAIRS = [
    pytest.param((480, 640), 136, 200, "model", 3, 1, True, id="480p-b136-model-L3-1slice-overlap"),
    pytest.param((480, 640), 136, 200, "rotation", 0, 2, False, id="480p-b136-rotation-L0-2slices"),
    pytest.param((480, 640), 256, 120, "model", 1, 2, True, id="480p-b256-model-L1-2slices-overlap"),
    pytest.param((480, 640), 24, 200, "model", 0, 1, False, id="480p-b24-model-L0-1slice"),
    pytest.param((480, 640), 24, 200, "rotation", 1, 2, True, id="480p-b24-rotation-L1-2slices-overlap"),
    pytest.param((480, 640), 127, 200, "rotation", 3, 1, False, id="480p-b127-rotation-L3-1slice"),
    pytest.param((1080, 1920), 8, 500, "model", 3, 1, True, id="1080p-b8-model-L3-1slice-overlap"),
    pytest.param((1080, 1920), 8, 500, "rotation", 0, 2, False, id="1080p-b8-rotation-L0-2slices"),
    pytest.param((1080, 1920), 130, 300, "model", 1, 1, True, id="1080p-b130-model-L1-1slice-overlap"),
    pytest.param((1080, 1920), 12, 500, "model", 0, 2, True, id="1080p-b12-model-L0-2slices-overlap"),
]


@pytest.mark.parametrize("shape,B,corners,mode,L,slices,overlap", PAIRS)
def test_pairs_run_seeded(pkg, ofk, shape, B, corners, mode, L, slices, overlap):
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    h, w = shape
    prev, nxt, base = batch_frames(h, w, B)
    p0 = base[0]
    gain = 1.0 if mode == "model" else 0.75                      # a gain other than 1 travels through the setter too
    cfg = PipelineConfig(max_corners=corners, quality=0.01, min_distance=10, block_size=7, win=15, max_level=L, max_count=20, eps=0.03,
                         lk_seed=mode, seed_gain=gain)
    sensors = ofk.make_sensors(B, d=p0["d"], normal=p0["n"], omega=p0["omega"], scaling=p0["scaling"], cx=p0["cx"], cy=p0["cy"], v_prior=p0["v"])
    pipe = FlowPipeline(w, h, B, cfg, streams=slices)
    try:
        pipe.ctx.set_overlap(overlap)
        assert pipe.ctx.get_lk_seed() == (ofk.SEED_MODES[mode], gain)
        pipe.upload(prev, nxt, sensors)
        out = pipe.run()
        compare_pairs(ofk, pipe.ctx, out, prev, nxt, sensors, cfg, ofk.SEED_MODES[mode], gain, "first run")
        if B <= 24:                                              # a second call on the resident pairs (the other pyramid set under overlap)
            out2 = pipe.run()
            for k in ("prev_pts", "next_pts", "status", "err", "counts"):
                assert np.array_equal(bits(out2[k]), bits(out[k])), k
            assert np.array_equal(out2["records"].view(np.uint64), out["records"].view(np.uint64))
    finally:
        pipe.close()


@pytest.fixture(scope="module")
def exp_pipe(pkg, ofk):
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    cfg = PipelineConfig(max_corners=300, quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)
    pipe = FlowPipeline(R.W_EXP, R.H_EXP, 1, cfg)
    yield pipe
    pipe.close()


@pytest.mark.parametrize("row", R.ROWS, ids=[r[0] for r in R.ROWS])
def test_fast_manoeuvre_rows_on_the_device(pkg, ofk, exp_pipe, row):
    from of_amd.pipeline import PipelineConfig
    name, v, omega, expect, inside, _ = row
    e = R.experiment_pair(name)
    pair = e["pair"]
    sensors = R.experiment_sensors(pair)[None]
    ctx = exp_pipe.ctx
    ctx.pairs_upload(pair["prev"][None], pair["next"][None]); ctx.pairs_set_sensors(sensors)

    def run(mode, L):
        cfg = PipelineConfig(max_corners=300, quality=0.01, min_distance=10, block_size=7, win=15, max_level=L, max_count=20, eps=0.03)
        ctx.set_lk_seed(mode, 1.0)
        ctx.pairs_run(cfg.to_params())
        out = ctx.pairs_download()
        n = int(out["counts"][0])
        assert n == len(e["pts"]) and np.array_equal(out["prev_pts"][0, :n], e["pts"])
        good = R.good_points(e, out["next_pts"][0, :n], out["status"][0, :n])
        return good, float(np.linalg.norm(out["records"][0, :3] - pair["v"]))

    try:
        (p3, _), ev_plain3 = run("off", 3)
        (p0, _), _ = run("off", 0)
        (s0, ins), ev_seeded0 = run("model", 0)
        (r0, _), _ = run("rotation", 0)
    finally:
        ctx.set_lk_seed("off")
    print(f"{name}: plain L3 {p3}/{ins}, plain L0 {p0}/{ins}, seeded L0 {s0}/{ins}, rotation-seeded L0 {r0}/{ins}; "
          f"|v_obs - v| plain L3 {ev_plain3:.4f}, seeded L0 {ev_seeded0:.4f}")
    assert ins == inside
    assert s0 >= R.SEEDED_MIN_GOOD * ins
    if name in R.LARGE_MOTION:
        assert p0 <= R.PLAIN_MAX_GOOD * ins
    if name in R.ROTATION_ROWS:
        assert r0 >= R.SEEDED_MIN_GOOD * ins
    if name in ("pitchroll", "translation"):
        assert ev_seeded0 <= 0.25 * ev_plain3
    assert (p3, p0, s0) == expect                                # the device computes what the reference computes: the same counts


YAW = dict(v=(0.003, -0.002, 0.001), omega=(0.002, -0.001, 0.08), d=1.0)


@pytest.mark.parametrize("kind", ["step", "fused-sensors", "fused-imu"])
@pytest.mark.parametrize("mode", ["model", "rotation"])
def test_stream_steps_seeded(pkg, ofk, gpu_ctx, kind, mode):
    from of_amd import synth
    from of_amd.pipeline import FlowStream, PipelineConfig, FusionConfig
    h, w, nf, B = 480, 640, 6, 2
    cfg = PipelineConfig(max_corners=150, quality=0.02, min_distance=10, block_size=7, win=15, max_level=1, max_count=20, eps=0.03,
                         lk_seed=mode, seed_gain=1.0)
    seqs = [synth.render_sequence(h, w, 700 + b, nf, margin=200, **YAW) for b in range(B)]
    frames = np.stack([s[0] for s in seqs]); info = seqs[0][1]
    sensors = ofk.make_sensors(B, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"],
                               v_prior=info["v"])
    fusion = None if kind == "step" else FusionConfig(use_imu=False) if kind == "fused-sensors" else FusionConfig.node()
    min_feat, radius = 140, 15
    rng = np.random.default_rng(8)
    fs = FlowStream(w, h, batch=B, cfg=cfg, min_features=min_feat, mask_radius=radius, fusion=fusion)
    smode = ofk.SEED_MODES[mode]
    try:
        tracks, counts = fs.begin(frames[:, 0])
        loops = [NodeLoop(frames[b, 0], cfg, min_feat, radius) for b in range(B)]
        for b in range(B):
            assert counts[b] == len(loops[b].tracks) and np.array_equal(tracks[b, :counts[b]], loops[b].tracks)
        moved = redetected = 0
        for t in range(1, nf):
            src = sensors.copy()
            if kind == "fused-imu":
                fs.push_imu(np.stack([imu_messages(rng, 50.0 + 0.1 * t + 3 * b, 3, rate=YAW["omega"], rate_sigma=0.001) for b in range(B)]))
                st, _ = fs.ctx.imu_state(B)                     # what the step will read: normal 15..17, omega 18..20, velocity 0..2
                src[:, 1:4] = st[:, 15:18]; src[:, 4:7] = st[:, 18:21]; src[:, 22:25] = st[:, 0:3]
            old = np.zeros((B, cfg.max_corners, 2), np.float32)
            oc = np.array([len(l.tracks) for l in loops], np.int32)
            for b in range(B):
                old[b, :oc[b]] = loops[b].tracks
            seeds = gpu_ctx.predict_points(old, oc, src, smode, 1.0)             # another context: the predictor needs no resident state
            assert np.array_equal(bits(seeds), bits(fs.ctx.predict_points(old, oc, src, smode, 1.0)))
            if kind == "step":
                rec, tracks, counts = fs.step(frames[:, t], sensors)
            else:
                rec, fused, tracks, counts = fs.step_fused(frames[:, t], sensors)
            for b in range(B):
                sd = seeds[b, :oc[b]]
                lk = lambda g0, g1, o: R.lk_pyr(g0, g1, o, cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr, seed=sd, flags=R.USE_INITIAL_FLOW)
                moved += int(np.sum(np.abs(sd - old[b, :oc[b]]) > 2))
                o = loops[b].step(frames[b, t], src[b], lk=lk)
                v, tr, n_old, n_tr = o["v"], o["tracks"], o["n_old"], o["n_tracked"]
                assert rec[b, 12] == n_old and rec[b, 13] == n_tr and counts[b] == len(tr), (t, b, rec[b, 12:14], n_old, n_tr, counts[b], len(tr))
                assert np.array_equal(bits(tracks[b, :counts[b]]), bits(tr.astype(np.float32))), (t, b)
                if v is not None:
                    np.testing.assert_allclose(rec[b, :3], v, rtol=1e-8, atol=1e-12)
                redetected += int(len(tr) > n_tr)
                if kind != "fused-imu":                         # true sensors: the seeded tracker holds its points through a yaw of 0.08 per
                    assert n_tr >= 0.6 * n_old, (t, b, n_tr, n_old)      # frame on two levels (the dead-reckoned IMU velocity is not the truth)
        assert moved > 0
    finally:
        fs.close()


def test_seed_off_after_on_is_the_unseeded_context(pkg, ofk):
    from of_amd import synth
    from of_amd.pipeline import FlowPipeline, FlowStream, PipelineConfig
    h, w, B = 480, 640, 8
    prev, nxt, base = batch_frames(h, w, B)
    p0 = base[0]
    sensors = ofk.make_sensors(B, d=p0["d"], normal=p0["n"], omega=p0["omega"], scaling=p0["scaling"], cx=p0["cx"], cy=p0["cy"], v_prior=p0["v"])
    cfg = PipelineConfig(max_corners=200, quality=0.01, min_distance=10, block_size=7, win=15, max_level=2, max_count=20, eps=0.03)
    outs = []
    for touch in (False, True):
        pipe = FlowPipeline(w, h, B, cfg, streams=2)
        try:
            pipe.upload(prev, nxt, sensors)
            if touch:
                pipe.ctx.set_lk_seed("model", 1.0)
                seeded = pipe.run()
                pipe.ctx.set_lk_seed("off")
                assert pipe.ctx.get_lk_seed()[0] == ofk.SEED_OFF
            outs.append(pipe.run())
        finally:
            pipe.close()
    a, b = outs
    for k in ("prev_pts", "next_pts", "status", "err", "counts"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert np.array_equal(a["records"].view(np.uint64), b["records"].view(np.uint64))
    assert not np.array_equal(bits(seeded["next_pts"]), bits(b["next_pts"]))      # and the seeded run in between was a different run
    # the same for a stream
    frames, info = synth.render_sequence(h, w, 812, 4, margin=200, **YAW)
    s1 = ofk.make_sensors(1, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"], v_prior=info["v"])
    res = []
    for touch in (False, True):
        fs = FlowStream(w, h, batch=1, cfg=cfg, min_features=150, mask_radius=15)
        try:
            fs.begin(frames[None, 0])
            steps = []
            for t in range(1, 4):
                if touch and t == 1:
                    fs.ctx.set_lk_seed("rotation", 1.0)
                    fs.ctx.predict_points(np.zeros((1, 4, 2), np.float32), np.array([4], np.int32), s1, ofk.SEED_MODEL, 1.0)
                    fs.ctx.set_lk_seed("off")
                steps.append(fs.step(frames[None, t], s1))
            res.append(steps)
        finally:
            fs.close()
    for (r0, t0, c0), (r1, t1, c1) in zip(*res):
        assert np.array_equal(c0, c1) and np.array_equal(bits(t0), bits(t1)) and np.array_equal(r0.view(np.uint64), r1.view(np.uint64))
    pipe = FlowPipeline(w, h, 1, cfg)
    try:
        with pytest.raises(ofk.OfkError):
            pipe.ctx.set_lk_seed(7)
        with pytest.raises(ofk.OfkError):
            pipe.ctx.set_lk_seed("model", float("nan"))
        assert pipe.ctx.get_lk_seed() == (ofk.SEED_OFF, 1.0)
    finally:
        pipe.close()
