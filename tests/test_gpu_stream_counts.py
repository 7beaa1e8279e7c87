"""GPU: the stream lifecycle past one pass of 256 tracks per stream, and at no tracks at all, step by step against the restated
loops of tests/stream_oracle.py under the plans of tests/point_count_cases.py.

(a) 520-600 tracks (300 for the 256 boundary): k_update_tracks compacts three chunks with its running base, appends the re-detected
    corners up to the budget, and in the last two steps lands exactly on 512 (256) and on 513 (257) tracks; LK, the solve and the
    mask see the same counts.
(b) a stream that loses its texture for two frames: all tracks lost, steps with no tracks (LK, the solve and k_disc_mask on zero
    points, a re-detection that finds nothing), then the refill to max_corners - next to streams that re-detect a little and one
    that does not re-detect, in the same calls.
(c) mask_radius 0 and 255.
(d) step_fused with the three-state filter, the replace re-detection (k_replace_tracks), the track gate, the robust solve (plain step
    without drop, step_fused with drop) and LK seeded from the sensor model, over (a)'s first run and over (b).
(e) ofk_pairs_run with the robust solve on 600 corners per pair, workgroup form and wave form: the lanes' recomputed chunks.
Compared: tracks bit for bit, counts, record fields 12 and 13, v and v_uav at the stream tests' tolerances (rtol 1e-8, atol 1e-12)
on a solved step and zeros in fields 0-2 and 4 on an unsolved one; the variants' own outputs by the rules of their own test files.
tests/test_point_count_cases.py asserts on the reference alone that the plans reach what they are for."""
import dataclasses

import numpy as np
import pytest

from batch_oracle import assert_records_identical
import point_count_cases as P  # noqa: E402  (tests/point_count_cases.py)
from point_count_cases import bits
import test_gpu_robust_pipeline as RP  # noqa: E402  compare_pair: the pair comparison of the robust pipeline tests, allowances included

pytestmark = pytest.mark.gpu


def open_streams(ofk, cfg, max_pts, fusion):
    """What pipeline.FlowStream sets up, on a context that holds max_pts points per stream (a landing step asks for more corners
    than the run's own max_corners)."""
    from of_amd.pipeline import FilterModel
    ctx = ofk.Context(0, P.W, P.H, P.B_STREAMS, max_pts, cfg.max_level)
    if cfg.lk_seed != "off":
        ctx.set_lk_seed(cfg.lk_seed, cfg.seed_gain)
    if cfg.robust != "off":
        ctx.set_robust(cfg.robust_setting())
    if cfg.track_gate_setting() is not None:
        ctx.set_track_gate(cfg.track_gate_setting())
    if fusion is not None:
        ctx.imu_reset(P.B_STREAMS)
        if fusion.filter:
            ctx.filter_configure(fusion.model or FilterModel.kf3(), P.B_STREAMS)
    return ctx


def check_streams(ofk, kind, max_corners, min_features, radius=P.MASK_RADIUS, variant=None, drop=False, gpu_ctx=None):
    from of_amd.pipeline import FusionConfig
    seeds = None
    if variant == "seed":                                        # the device's predictor on another context, as tests/test_gpu_seed_pipeline.py has it
        seeds = lambda old, counts, sens: gpu_ctx.predict_points(old, counts, sens, ofk.SEED_MODEL, 1.0)
    run = P.stream_run(kind, max_corners, min_features, radius, variant, drop, seeds)
    frames, _ = P.stream_frames(kind == "zero")
    cfg, sensors, B = run["cfg"], run["sensors"], P.B_STREAMS
    fusion = P.kf3_fusion() if variant == "kf3" else FusionConfig(use_imu=False) if variant == "robust-fused" else None
    max_pts = max(max_corners, max(mc for mc, _ in run["asked"]))
    ctx = open_streams(ofk, cfg, max_pts, fusion)
    try:
        tracks, counts = ctx.stream_begin(frames[:, 0], cfg.to_params())
        for b in range(B):
            assert counts[b] == len(run["first"][b]) and np.array_equal(bits(tracks[b, :counts[b]]), bits(run["first"][b])), ("begin", b)
        for t, (mc, mf) in enumerate(run["asked"], start=1):
            params = dataclasses.replace(cfg, max_corners=mc).to_params()
            if fusion is not None:
                rec, fused, tracks, counts = ctx.stream_step_fused(frames[:, t], sensors, params, fusion.to_struct(), mf, radius)
            else:
                rec, tracks, counts = ctx.stream_step(frames[:, t], sensors, params, mf, radius)
            if variant == "gate":
                stats = ctx.track_gate_stats(B)
                nxt, keep = ctx.stream_last_points(max_pts)
            if variant in ("robust", "robust-fused"):
                wts, st = ctx.robust_download(B)
            for b in range(B):
                o = run["steps"][t - 1][b]; tag = (kind, max_corners, min_features, radius, variant, drop, "step", t, "stream", b, "asked", mc, mf)
                n_old = o["n_old"]
                assert rec[b, 12] == n_old and rec[b, 13] == o["n_tracked"] and counts[b] == len(o["tracks"]), \
                    (tag, rec[b, 12:14], n_old, o["n_tracked"], counts[b], len(o["tracks"]))
                bad = P.differing(tracks[b, :counts[b]], o["tracks"].astype(np.float32))
                assert bad.size == 0, (tag, "tracks: first differing index", int(bad[0]), "chunk", int(bad[0]) // 256, "of", bad.size)
                if o["solved"]:
                    np.testing.assert_allclose(rec[b, :3], o["v"], rtol=1e-8, atol=1e-12, err_msg=str(tag))
                    np.testing.assert_allclose(rec[b, 8:11], o["v_uav"], rtol=1e-8, atol=1e-12, err_msg=str(tag))
                else:
                    assert not rec[b, 0:3].any() and rec[b, 4] == 0, (tag, "an unsolved step", rec[b])
                if variant == "kf3":
                    np.testing.assert_allclose(fused[b, :3], o["x"], rtol=1e-8, atol=1e-12, err_msg=str(tag))
                    assert fused[b, 7] == (1 if o["solved"] else 0), (tag, fused[b])
                if variant == "gate":
                    r = o["gate"]
                    assert np.array_equal(stats[b], r["stats"]), (tag, stats[b], r["stats"])
                    assert np.array_equal(keep[b, :n_old], r["status"]) and np.array_equal(bits(nxt[b, :n_old]), bits(r["next"])), tag
                if variant in ("robust", "robust-fused"):
                    assert o["gap"] >= 1e-6 and o["near"] == 0, tag        # the conditions of tests/test_gpu_robust.py, on the reference
                    assert rec[b, 11] == o["used"], (tag, rec[b, 11], o["used"])
                    np.testing.assert_array_equal(st[b, [3, 4, 6, 7]], o["stats"][[3, 4, 6, 7]], err_msg=str(tag))
                    np.testing.assert_allclose(wts[b, :n_old], o["weights"], rtol=0, atol=1e-9, err_msg=str(tag))
    finally:
        ctx.close()
    return run


EDGE_RUNS = [pytest.param(mc, mf, id=f"{mc}-{mf}") for mc, mf in P.RUNS]


@pytest.mark.parametrize("max_corners,min_features", EDGE_RUNS)
def test_stream_chunk_edges(pkg, ofk, max_corners, min_features):
    check_streams(ofk, "edges", max_corners, min_features)


def test_stream_at_zero_tracks(pkg, ofk):
    check_streams(ofk, "zero", 600, 590)


@pytest.mark.parametrize("max_corners,min_features,radius", [(600, 590, 0), (300, 256, 0), (600, 590, 255)], ids=["600-r0", "300-r0", "600-r255"])
def test_stream_mask_radius(pkg, ofk, max_corners, min_features, radius):
    run = check_streams(ofk, "edges", max_corners, min_features, radius=radius)
    if radius == 255:                                            # every disc covers the frame: the streams re-detect and find nothing
        steps = [o for row in run["steps"] for o in row]
        assert all(len(o["tracks"]) == o["n_tracked"] for o in steps) and any(o["n_old"] <= 590 for o in steps)


VARIANTS = [("kf3", False), ("gate", False), ("robust", False), ("robust-fused", True), ("seed", False)]


@pytest.mark.parametrize("kind", ["edges", "zero"])
@pytest.mark.parametrize("variant,drop", VARIANTS, ids=["kf3", "gate-seeded-L0", "robust-step-keep", "robust-fused-drop", "lk-seed-model"])
def test_stream_variants(pkg, ofk, gpu_ctx, kind, variant, drop):
    check_streams(ofk, kind, 600, 590, variant=variant, drop=drop, gpu_ctx=gpu_ctx)


@pytest.mark.parametrize("kind", ["edges", "zero"])
def test_stream_replace_redetection(pkg, ofk, kind):
    """step_fused as the loop of of_module.py (k_replace_tracks in front of LK) against stream_oracle.oracle_of_module, at the
    tolerances of tests/test_gpu_fused.py."""
    from of_amd.pipeline import FusionConfig
    m = P.module_run(kind)
    frames, _ = P.stream_frames(kind == "zero")
    cfg, B = P.module_cfg(), P.B_STREAMS
    fusion = FusionConfig.of_module(synthetic_flow=False)
    ctx = open_streams(ofk, cfg, cfg.max_corners, fusion)
    try:
        tracks, counts = ctx.stream_begin(frames[:, 0], cfg.to_params())
        for b in range(B):
            assert counts[b] == len(m["refs"][b][0]) and np.array_equal(bits(tracks[b, :counts[b]]), bits(m["refs"][b][0]))
        for t in range(1, P.NF):
            sensors = np.concatenate([ofk.make_sensors(1, d=1.0, normal=m["normal"], omega=m["omegas"][t - 1, b], scaling=1.0, cx=m["cx"], cy=m["cy"])
                                      for b in range(B)])
            sensors[:, 25:28] = m["controls"][t - 1]
            rec, fused, tracks, counts = ctx.stream_step_fused(frames[:, t], sensors, cfg.to_params(), fusion.to_struct(), P.MODULE_MIN_FEATURES,
                                                               P.MASK_RADIUS)
            for b in range(B):
                v, xk, Pk, tr, n_old, n_keep = m["refs"][b][1][t - 1]; tag = ("replace", kind, "step", t, "stream", b)
                assert rec[b, 12] == n_old and rec[b, 11] == n_keep and counts[b] == len(tr), (tag, rec[b, 11:14], n_old, n_keep, len(tr))
                bad = P.differing(tracks[b, :counts[b]], tr.astype(np.float32))
                assert bad.size == 0, (tag, "tracks: first differing index", int(bad[0]), "of", bad.size)
                if v is not None:
                    np.testing.assert_allclose(rec[b, :3], v, rtol=1e-7, atol=1e-12, err_msg=str(tag))
                    assert rec[b, 15] == 1 and fused[b, 7] == 1, tag
                else:
                    assert rec[b, 15] == 0 and rec[b, 4] == 0 and not rec[b, 0:3].any(), (tag, rec[b])
                np.testing.assert_allclose(fused[b, :3], xk, rtol=1e-8, atol=1e-12, err_msg=str(tag))
                np.testing.assert_allclose(fused[b, 6], np.trace(Pk), rtol=1e-10, err_msg=str(tag))
    finally:
        ctx.close()


def run_pairs(ofk, B):
    from of_amd.pipeline import FlowPipeline
    info, prev, nxt = P.pair_scenes()
    idx = np.arange(B) % len(prev)
    sensors = ofk.make_sensors(B, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"])
    pipe = FlowPipeline(P.W, P.H, B, P.pair_cfg(), streams=1)
    try:
        pipe.ctx.set_robust(**P.PAIR_SETTING)
        pipe.upload(prev[idx], nxt[idx], sensors)
        out = pipe.run()
        wts, st = pipe.ctx.robust_download(B)
    finally:
        pipe.close()
    return sensors, out, wts, st


def test_pairs_run_robust_past_512_points(pkg, ofk):
    """A lane of the robust solve keeps rho^2 of its first eight chunks of 64 points and recomputes the rest: 600 corners per pair make
    it recompute, in the workgroup form (4 pairs) and in the wave form (128 pairs: the 4 scenes repeated, another sample each)."""
    before = dict(RP.USED)
    runs = {}
    for B in (4, 128):
        sensors, out, wts, st = run_pairs(ofk, B)
        assert np.all(out["counts"] == P.PAIR_CORNERS), out["counts"]
        for b in range(B):
            RP.compare_pair(out, b, sensors[b], wts[b], st[b], P.PAIR_SETTING, f"B {B} pair {b}")
            late = np.arange(P.PAIR_CORNERS) >= 512
            assert np.count_nonzero((wts[b] == 0) & late & (out["status"][b] == 1)) >= 5 and np.count_nonzero((wts[b] > 0) & late) >= 5, (B, b)
        runs[B] = (out["records"], wts, st)
    for name, a, b in zip(("records", "weights", "stats"), runs[4], runs[128]):
        assert_records_identical(a, b[:4], f"workgroup form against wave form: {name}")
    cases, hyp, count = (RP.USED[k] - before[k] for k in ("cases", "hyp", "count"))
    print(f"pairs past 512 points: {cases} cases, allowances used: hyp {hyp}, count {count}")
    assert hyp <= 0.01 * cases and count <= 0.01 * cases, (cases, hyp, count)
