"""GPU: the robust-solve setting (ofk_set_robust) through ofk_pairs_run and the stream steps, against the test-side reference
(tests/robust_reference.py) fed with the downloaded points and status.

(1) ofk_pairs_run with the setting on: every pair's record, weights and stats; image outputs bit-identical to the plain run.
(2) launch-form identity: the same pairs through the workgroup form (B = 24) and the wave form (B = 136), one and two slices.
(3) off after on: bit-identical to a context that never had the setting; invalid settings raise and change nothing.
(4) the moving-object experiment end to end on the device, held to the conditions of tests/robust_reference.py.
(5) FlowStream.step / step_fused (sensors; resident IMU state with the ekf6 filter) against the restated loop of
    tests/robust_stream_oracle.py, drop off and on."""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from batch_oracle import assert_records_identical
from oracle import estimation_oracle as eo
from point_stage_helpers import bits
import robust_reference as rr
import robust_stream_oracle as rso
from stream_oracle import NodeLoop, imu_messages

pytestmark = pytest.mark.gpu

MOTION = dict(v=(0.004, -0.003, 0.002), omega=(0.003, -0.002, 0.004), d=1.0)
MAX_BATCH = {(480, 640): 256, (1080, 1920): 130}                                  # rendered once per size
SETTING = dict(loss="tukey", c=4.685, iters=5, hypotheses=64, seed=0x1234ABCD5678)
_batches = {}
USED = dict(cases=0, hyp=0, count=0)
USED_LOCK = threading.Lock()                                    # compare_pair runs on a thread pool


def batch_frames(h, w, B):
    key = (h, w)
    if key not in _batches:
        from of_amd import synth
        prev, nxt, base = synth.make_batch(MAX_BATCH[key], h, w, seed=4100, distinct=4, margin=96, **MOTION)
        prev, nxt = prev.copy(), nxt.copy()
        for b in range(1, len(prev), 2):                        # every other pair carries an object that moves by (-7, +5) px on its own
            oh, ow = rr.OBJECT_SIZES[(b // 2) % 3]
            tex = synth.render_pair(oh + 40, ow + 40, 5000 + b % 7, margin=96)["prev"][20:20 + oh, 20:20 + ow]
            prev[b, 60:60 + oh, 80:80 + ow] = tex; nxt[b, 65:65 + oh, 73:73 + ow] = tex
        _batches[key] = (prev, nxt, base)
    prev, nxt, base = _batches[key]
    return prev[:B], nxt[:B], base


def compare_pair(out, b, sr, w, st, setting, tag):
    """Pair b's record, weights and stats against the reference on the downloaded points and status (the allowances of
    tests/test_gpu_robust.py)."""
    n = int(out["counts"][b])
    new = out["next_pts"][b, :n].astype(np.float64); old = out["prev_pts"][b, :n].astype(np.float64)
    ok = out["status"][b, :n] == 1
    x = (new - [sr[20], sr[21]]) * sr[19]; u = (new - old) * sr[19]
    kw = dict(valid=ok, loss=rr.TUKEY if setting["loss"] == "tukey" else rr.HUBER, c=setting["c"], iters=setting["iters"],
              hypotheses=setting["hypotheses"], seed=setting["seed"], problem=b)
    ref = rr.robust_solve(rr.NODE, x, u, sr[0], sr[1:4], sr[4:7], **kw)
    with USED_LOCK:
        USED["cases"] += 1
    if int(st[4]) != int(ref["stats"][4]):
        best = ref["stats"][5]
        assert int(st[4]) >= 0 and abs(st[5] - best) <= 1e-12 * best, (tag, "hyp", st, ref["stats"])
        with USED_LOCK:
            USED["hyp"] += 1
        ref = rr.robust_solve(rr.NODE, x, u, sr[0], sr[1:4], sr[4:7], force_hyp=int(st[4]), **kw)
    rec, rs = out["records"][b], ref["stats"]
    assert (int(rec[4]), int(st[3]), int(st[4]), int(st[6]), int(st[7])) == (ref["rank"], int(rs[3]), int(rs[4]), int(rs[6]), int(rs[7])), (tag, rec, st, rs)
    assert rec[12] == n and rec[13] == int(ok.sum()) and rec[11] == st[2], (tag, rec[11:14])
    if st[2] != rs[2]:
        assert kw["loss"] == rr.TUKEY and abs(st[2] - rs[2]) <= ref["near"], (tag, "count", st[2], rs[2])
        with USED_LOCK:
            USED["count"] += 1
    np.testing.assert_allclose(rec[0:3], ref["v"], rtol=1e-9, atol=1e-13, err_msg=tag)
    np.testing.assert_allclose(rec[5:8], ref["s"], rtol=1e-9, err_msg=tag)
    np.testing.assert_allclose(rec[3], ref["r"], rtol=1e-6, atol=1e-18, err_msg=tag)
    np.testing.assert_allclose(rec[8:11], eo.post_solve(ref["v"], sr[7:16].reshape(3, 3), sr[4:7], sr[16:19]), rtol=1e-9, atol=1e-13, err_msg=tag)
    np.testing.assert_allclose(st[[0, 5]], rs[[0, 5]], rtol=1e-9, err_msg=tag)
    np.testing.assert_allclose(st[1], rs[1], rtol=1e-9, err_msg=tag)
    np.testing.assert_allclose(w[:n], ref["weights"], rtol=0, atol=1e-9, err_msg=tag)
    assert not w[n:].any(), tag
    return ref


def run_pairs(ofk, shape, B, corners, slices, overlap, setting, frames=None):
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    h, w = shape
    prev, nxt, base = frames if frames is not None else batch_frames(h, w, B)
    p0 = base[0]
    cfg = PipelineConfig(max_corners=corners, quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)
    sensors = ofk.make_sensors(B, d=p0["d"], normal=p0["n"], omega=p0["omega"], scaling=p0["scaling"], cx=p0["cx"], cy=p0["cy"], v_prior=p0["v"])
    pipe = FlowPipeline(w, h, B, cfg, streams=slices)
    try:
        pipe.ctx.set_overlap(overlap)
        pipe.upload(prev, nxt, sensors)
        plain = pipe.run()
        pipe.ctx.set_robust(**setting)
        out = pipe.run()
        wts, st = pipe.ctx.robust_download(B)
        pipe.ctx.set_robust(None)
        again = pipe.run()
    finally:
        pipe.close()
    return sensors, plain, out, wts, st, again


# size, batch, corners, slices, overlap.  One wave per pair from 128 pairs per slice on, a workgroup per pair below.
PAIRS = [
    pytest.param((480, 640), 24, 300, 1, False, id="480p-b24-1slice"),
    pytest.param((480, 640), 24, 300, 2, True, id="480p-b24-2slices-overlap"),
    pytest.param((480, 640), 127, 200, 1, True, id="480p-b127-1slice-overlap"),
    pytest.param((480, 640), 136, 200, 1, False, id="480p-b136-1slice"),
    pytest.param((480, 640), 136, 200, 2, True, id="480p-b136-2slices-overlap"),
    pytest.param((480, 640), 256, 150, 1, True, id="480p-b256-1slice-overlap"),
    pytest.param((480, 640), 256, 150, 2, False, id="480p-b256-2slices"),
    pytest.param((1080, 1920), 8, 500, 1, True, id="1080p-b8-1slice-overlap"),
    pytest.param((1080, 1920), 8, 500, 2, False, id="1080p-b8-2slices"),
    pytest.param((1080, 1920), 130, 300, 1, True, id="1080p-b130-1slice-overlap"),
    pytest.param((1080, 1920), 130, 300, 2, False, id="1080p-b130-2slices"),
]


@pytest.mark.parametrize("shape,B,corners,slices,overlap", PAIRS)
def test_pairs_run_robust(pkg, ofk, shape, B, corners, slices, overlap):
    sensors, plain, out, wts, st, again = run_pairs(ofk, shape, B, corners, slices, overlap, SETTING)
    for k in ("prev_pts", "next_pts", "status", "err", "counts"):            # the image stages do not know the setting
        assert np.array_equal(bits(out[k]), bits(plain[k])), k
        assert np.array_equal(bits(again[k]), bits(plain[k])), k
    assert_records_identical(again["records"], plain["records"], "off after on")
    assert not np.array_equal(bits(out["records"][:, :3]), bits(plain["records"][:, :3]))
    with ThreadPoolExecutor(16) as ex:
        refs = list(ex.map(lambda b: compare_pair(out, b, sensors[b], wts[b], st[b], SETTING, f"{shape} B {B} slices {slices} pair {b}"), range(B)))
    moved = sum(1 for b in range(B) if np.linalg.norm(out["records"][b, :3] - plain["records"][b, :3]) > 0.2 * np.linalg.norm(MOTION["v"]))
    print(f"{shape} B {B}: pairs whose velocity moved by more than 20 %: {moved}; zero-weight points: {int(np.sum((wts == 0) & (out['status'] == 1)))}")
    assert len(refs) == B and np.any((wts == 0) & (out["status"] == 1))       # the reweighting rejected points
    if shape == (480, 640):                                       # there the objects cover 10-40 % of the corners (a few % at 1080p)
        assert moved >= B // 4


def test_launch_forms_and_slices_give_the_same_bits(pkg, ofk):
    prev, nxt, base = batch_frames(480, 640, 136)
    runs = {}
    for B, slices in ((24, 1), (136, 1), (136, 2), (24, 2)):
        _, _, out, wts, st, _ = run_pairs(ofk, (480, 640), B, 200, slices, True, SETTING, frames=(prev[:B], nxt[:B], base))
        runs[(B, slices)] = (out["records"], wts, st)
    ref = runs[(136, 1)]
    for key, (rec, wts, st) in runs.items():
        B = key[0]
        assert_records_identical(rec, ref[0][:B], f"records {key}")
        assert_records_identical(wts, ref[1][:B], f"weights {key}")
        assert_records_identical(st, ref[2][:B], f"stats {key}")


def test_off_after_on_and_invalid_settings(pkg, ofk):
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
                pipe.ctx.set_robust(**SETTING)
                robust = pipe.run()
                pipe.ctx.set_robust(loss="off")
                assert pipe.ctx.get_robust().loss == ofk.ROBUST_OFF
            outs.append(pipe.run())
        finally:
            pipe.close()
    a, b = outs
    for k in ("prev_pts", "next_pts", "status", "err", "counts"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert_records_identical(a["records"], b["records"], "pipeline off after on")
    assert not np.array_equal(bits(robust["records"]), bits(b["records"]))
    # the same for a stream, drop included: nothing of it survives the switch
    frames, info = rso.sequence(synth, h, w, 812, 4)
    s1 = ofk.make_sensors(1, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"], v_prior=info["v"])
    res = []
    for touch in (False, True):
        fs = FlowStream(w, h, batch=1, cfg=cfg, min_features=150, mask_radius=15)
        try:
            fs.begin(frames[None, 0])
            steps = []
            for t in range(1, 4):
                if touch and t == 1:
                    fs.ctx.set_robust(drop=True, **SETTING)
                    fs.ctx.set_robust(None)
                steps.append(fs.step(frames[None, t], s1))
            res.append(steps)
        finally:
            fs.close()
    for (r0, t0, c0), (r1, t1, c1) in zip(*res):
        assert np.array_equal(c0, c1) and np.array_equal(bits(t0), bits(t1))
        assert_records_identical(r0, r1, "stream off after on")
    pipe = FlowPipeline(w, h, 1, cfg)
    try:
        good = dict(SETTING, hypotheses=16, iters=3)
        pipe.ctx.set_robust(**good)
        for bad in (dict(loss=3), dict(c=0.0), dict(c=-1.0), dict(c=float("nan")), dict(c=float("inf")), dict(iters=-1), dict(iters=33),
                    dict(hypotheses=-1), dict(hypotheses=257)):
            with pytest.raises(ofk.OfkError):
                pipe.ctx.set_robust(**dict(good, **bad))
        r = ofk.robust_setting(**good); r.drop = 2
        with pytest.raises(ofk.OfkError):
            pipe.ctx.set_robust(r)
        g = pipe.ctx.get_robust()                                # the previous setting is still in place
        assert (g.loss, g.c, g.iters, g.hypotheses, g.seed, g.drop) == (2, 4.685, 3, 16, SETTING["seed"], 0)
        with pytest.raises(ofk.OfkError):
            pipe.ctx.robust_download(1)                          # nothing has run with the setting on yet
    finally:
        pipe.close()


@pytest.mark.parametrize("size", rr.OBJECT_SIZES + (None,), ids=lambda s: "none" if s is None else f"{s[0]}x{s[1]}")
def test_moving_object_experiment_on_the_device(pkg, ofk, size):
    from of_amd import synth
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    cfg = PipelineConfig(max_corners=300, quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)
    scenes = [rr.scene(synth, seed, size) for seed in rr.SCENE_SEEDS]
    B = len(scenes)
    p0 = scenes[0][0]
    sensors = ofk.make_sensors(B, d=p0["d"], normal=p0["n"], omega=p0["omega"], scaling=p0["scaling"], cx=p0["cx"], cy=p0["cy"])
    setting = dict(loss="tukey", c=rr.EXPERIMENT["c"], iters=rr.EXPERIMENT["iters"], hypotheses=rr.EXPERIMENT["hypotheses"], seed=rr.EXPERIMENT["seed"])
    pipe = FlowPipeline(640, 480, B, cfg)
    try:
        pipe.upload(np.stack([s[1] for s in scenes]), np.stack([s[2] for s in scenes]), sensors)
        plain = pipe.run()
        pipe.ctx.set_robust(**setting)
        out = pipe.run()
        wts, st = pipe.ctx.robust_download(B)
    finally:
        pipe.close()
    for b, (pair, _, _) in enumerate(scenes):
        # problem b of a batch of scenes draws another sample than problem 0 of the CPU experiment: the reference is re-run with it
        ref = compare_pair(out, b, sensors[b], wts[b], st[b], setting, f"scene {size} seed {rr.SCENE_SEEDS[b]}")
        ep, er = rr.rel_err(plain["records"][b, :3], pair["v"]), rr.rel_err(out["records"][b, :3], pair["v"])
        n = int(out["counts"][b])
        obj = rr.on_object(out["prev_pts"][b, :n], size) & (out["status"][b, :n] == 1)
        print(f"object {size} seed {rr.SCENE_SEEDS[b]}: share {obj.sum() / max(1, (out['status'][b, :n] == 1).sum()):.2f} plain {ep:.4f} robust {er:.4f} "
              f"(reference {rr.rel_err(ref['v'], pair['v']):.4f}) object corners with w > 0: {int(np.count_nonzero(wts[b, :n][obj] > 0))}")
        rr.check_experiment(size, ep, er, (size, rr.SCENE_SEEDS[b]))


@pytest.mark.parametrize("drop", [False, True], ids=["keep", "drop"])
@pytest.mark.parametrize("kind", ["step", "fused", "ekf6"])
def test_stream_steps_robust(pkg, ofk, kind, drop):
    from of_amd import synth
    from of_amd.pipeline import FlowStream, PipelineConfig, FusionConfig
    h, w, nf, B = 480, 640, 6, 2
    cfg = PipelineConfig(max_corners=200, quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03,
                         robust="tukey", robust_c=rso.SETTING["c"], robust_iters=rso.SETTING["iters"], robust_hypotheses=rso.SETTING["hypotheses"],
                         robust_seed=rso.SETTING["seed"], robust_drop=drop)
    seqs = [rso.sequence(synth, h, w, 900 + b, nf) for b in range(B)]
    frames = np.stack([s[0] for s in seqs]); info = seqs[0][1]
    sensors = ofk.make_sensors(B, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"])
    fusion = None if kind == "step" else FusionConfig(use_imu=False) if kind == "fused" else FusionConfig.ekf6(dt=0.1)
    min_feat, radius = 150, 15
    rng = np.random.default_rng(8)
    fs = FlowStream(w, h, batch=B, cfg=cfg, min_features=min_feat, mask_radius=radius, fusion=fusion)
    share = []
    try:
        tracks, counts = fs.begin(frames[:, 0])
        loops = [NodeLoop(frames[b, 0], cfg, min_feat, radius, solve=rso.robust_solver(b, drop, kind != "step"),
                          **(dict(imu_offset=(0.0, 0.0, 0.1), model=fusion.model) if kind == "ekf6" else {})) for b in range(B)]
        for b in range(B):
            assert counts[b] == len(loops[b].tracks) and np.array_equal(tracks[b, :counts[b]], loops[b].tracks)
        dropped = 0
        for t in range(1, nf):
            msgs = None
            if kind == "ekf6":
                msgs = np.stack([imu_messages(rng, 50.0 + 0.1 * t + 3 * b, 3, rate=MOTION["omega"], rate_sigma=0.0005) for b in range(B)])
                fs.push_imu(msgs)
            if kind == "step":
                rec, tracks, counts = fs.step(frames[:, t], sensors)
            else:
                rec, fused, tracks, counts = fs.step_fused(frames[:, t], sensors)
            wts, st = fs.ctx.robust_download(B)
            for b in range(B):
                o = loops[b].step(frames[b, t], sensors[b], () if msgs is None else msgs[b])
                tag = (kind, drop, t, b)
                assert o["gap"] >= 1e-6 and o["near"] == 0, tag
                assert rec[b, 12] == o["n_old"] and rec[b, 13] == o["n_tracked"] and rec[b, 11] == o["used"] and counts[b] == len(o["tracks"]), \
                    (tag, rec[b, 11:14], o["n_old"], o["n_tracked"], o["used"], counts[b], len(o["tracks"]))
                assert np.array_equal(bits(tracks[b, :counts[b]]), bits(o["tracks"].astype(np.float32))), tag
                np.testing.assert_allclose(rec[b, :3], o["v"], rtol=1e-8, atol=1e-12, err_msg=str(tag))
                np.testing.assert_allclose(rec[b, 8:11], o["v_uav"], rtol=1e-8, atol=1e-12, err_msg=str(tag))
                np.testing.assert_array_equal(st[b, [3, 4, 6, 7]], o["stats"][[3, 4, 6, 7]], err_msg=str(tag))
                np.testing.assert_allclose(wts[b, :o["n_old"]], o["weights"], rtol=0, atol=1e-9, err_msg=str(tag))
                if kind != "step":
                    assert rec[b, 15] == 1 and fused[b, 7] == 1, tag
                if kind == "ekf6":
                    np.testing.assert_allclose(fused[b, :6], o["x"], rtol=1e-8, atol=1e-12, err_msg=str(tag))
                    np.testing.assert_allclose(fused[b, 6], np.trace(o["P"]), rtol=1e-10, err_msg=str(tag))
                else:
                    assert rr.rel_err(rec[b, :3], info["v"]) <= rr.ROBUST_MAX, tag     # true sensors: the object does not drag the estimate
                dropped += int(np.count_nonzero((o["weights"] == 0) & (wts[b, :o["n_old"]] == 0))) - (o["n_old"] - o["n_tracked"])
        if kind == "ekf6":
            gx, gP = fs.ctx.filter_state(B)
            for b in range(B):
                np.testing.assert_allclose(gx[b], loops[b].x, rtol=1e-8, atol=1e-12)
                np.testing.assert_allclose(gP[b], loops[b].P, rtol=1e-10, atol=1e-14)
        share = [float(np.mean(rso.on_object(tracks[b, :counts[b]], nf - 1))) for b in range(B)]
        print(f"{kind} drop {drop}: share of tracks on the object after the last frame {share}, zero-weight tracked points over the run {dropped}")
        assert dropped > 0
        if drop and kind != "ekf6":
            assert max(share) < 0.05                            # the restated loop's figure (robust_stream_oracle.py): nothing is left on it
    finally:
        fs.close()


def test_without_hypotheses_and_rounds_the_robust_kernels_are_the_plain_ones(pkg, ofk):
    """K = 0, iters = 0: the start is the plain solve and every weight 1, so the robust kernels - k_stream_fuse_robust, the twin of
    k_stream_fuse, among them - must give the plain kernels' records, filter states and tracks bit for bit."""
    from of_amd import synth
    from of_amd.pipeline import FlowStream, PipelineConfig, FusionConfig
    null = dict(loss="tukey", c=4.685, iters=0, hypotheses=0, seed=1)
    for B in (24, 136):                                          # workgroup and wave form
        _, plain, out, wts, st, _ = run_pairs(ofk, (480, 640), B, 200, 1, True, null)
        assert_records_identical(out["records"], plain["records"], f"pairs B {B}")
        assert np.array_equal(wts > 0, (out["status"] == 1) & (np.arange(wts.shape[1])[None] < out["counts"][:, None]))
    h, w, nf, B = 480, 640, 5, 2
    seqs = [rso.sequence(synth, h, w, 900 + b, nf) for b in range(B)]
    frames = np.stack([s[0] for s in seqs]); info = seqs[0][1]
    sensors = ofk.make_sensors(B, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"], v_prior=info["v"])
    for name, fusion, pc in (("sensors", lambda: FusionConfig(use_imu=False), {}), ("node", FusionConfig.node, dict(use_feasibility=True, feas_T=0.5)),
                             ("ekf6", lambda: FusionConfig.ekf6(dt=0.1), {})):
        runs = []
        for robust in (False, True):
            cfg = PipelineConfig(max_corners=200, quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03, **pc)
            fs = FlowStream(w, h, batch=B, cfg=cfg, min_features=150, mask_radius=15, fusion=fusion())
            rng = np.random.default_rng(8)
            try:
                if robust:
                    fs.ctx.set_robust(**null)
                fs.begin(frames[:, 0])
                steps = []
                for t in range(1, nf):
                    if name != "sensors":
                        fs.push_imu(np.stack([imu_messages(rng, 50.0 + 0.1 * t + 3 * b, 3, rate=MOTION["omega"], rate_sigma=0.0005) for b in range(B)]))
                    steps.append(fs.step_fused(frames[:, t], sensors))
                runs.append((steps, fs.ctx.filter_state(B) if name == "ekf6" else None, fs.ctx.imu_state(B)))
            finally:
                fs.close()
        (sa, fa, ia), (sb, fb, ib) = runs
        for t, ((r0, f0, t0, c0), (r1, f1, t1, c1)) in enumerate(zip(sa, sb)):
            assert_records_identical(r0, r1, f"{name} records step {t}")
            assert_records_identical(f0, f1, f"{name} fused step {t}")
            assert np.array_equal(c0, c1) and np.array_equal(bits(t0), bits(t1)), (name, t)
        if fa is not None:
            assert_records_identical(fa[0], fb[0], "filter x"); assert_records_identical(fa[1], fb[1], "filter P")
        assert_records_identical(ia[0], ib[0], f"{name} imu state")


def test_the_allowances_stayed_rare():
    """Over whatever part of this module ran in this process."""
    print("cases", USED)
    assert USED["hyp"] <= 0.01 * max(USED["cases"], 1) and USED["count"] <= 0.01 * max(USED["cases"], 1), USED
