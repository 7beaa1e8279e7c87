"""GPU: the lighting-insensitive LK as a context setting (ofk_set_lk_light) through ofk_pairs_run and the stream steps.

(a) FlowPipeline (two slices) with lk_light on: every pair equals the composition of stage entries - the corners, ofk_lk_pyr_light
    (the gates behind it where the configuration has them) and the solve - and the test-side chain (tests/lk_light_reference.py).
(b) FlowStream.step / step_fused under exposure that changes from frame to frame, against the restated stream loop with the light's
    tracker plugged in; once beside lk_seed="model" and a forward-backward gate.
(c) the setting off after having been on: bit-identical to a context that never saw it.
(d) the exposure experiment end to end on the device, held to the bounds of tests/test_lk_light_reference.py."""
import numpy as np
import pytest

import lk_seed_reference as R  # noqa: E402  (tests/lk_seed_reference.py)
import lk_light_reference as LR  # noqa: E402  (tests/lk_light_reference.py)
import track_gate_reference as G  # noqa: E402  (tests/track_gate_reference.py)
from batch_oracle import assert_pair_matches, assert_records_identical  # noqa: E402  (tests/batch_oracle.py)
from stream_oracle import NodeLoop  # noqa: E402  (tests/stream_oracle.py)

pytestmark = pytest.mark.gpu

H, W = 240, 320
MOTION = dict(v=(0.003, -0.002, 0.001), omega=(0.03, -0.02, 0.1))
STREAM_MOTION = dict(v=(0.003, -0.002, 0.001), omega=(0.015, -0.01, 0.05), d=1.0)
CORNERS = dict(max_corners=60, quality=0.01, min_distance=5, block_size=5)
LK = dict(max_level=2, max_count=20, eps=0.03, min_eig_thr=1e-4)
PLAIN_GATE = dict(fb="plain", fb_thr=0.5, fb_level=-1, err_max=0.0)
# exposure of the next frame of pair b / of frame t of a stream: (gain, bias, vignette)
EXPOSURES = ((1.25, 10.0, 0.0), (0.75, -5.0, 0.3), (1.0, 0.0, 0.0), (1.1, 6.0, 0.2), (0.85, 0.0, 0.0), (1.2, -8.0, 0.1))
_pairs = {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def pairs(B):
    """B rendered BGR pairs, the next frame of pair b under EXPOSURES[b]."""
    if B not in _pairs:
        from of_amd import synth
        ps = [synth.render_pair(H, W, 5 + b, margin=64, **MOTION) for b in range(B)]
        prev = np.stack([p["prev"] for p in ps])
        nxt = np.stack([synth.apply_exposure(p["next"], *EXPOSURES[b % len(EXPOSURES)]) for b, p in enumerate(ps)])
        _pairs[B] = (prev, nxt, ps[0])
    return _pairs[B]


def config(win, light, gate=None, **kw):
    from of_amd.pipeline import PipelineConfig
    g = gate or G.OFF
    return PipelineConfig(win=win, lk_light=light, fb_check=g["fb"], fb_thr=g["fb_thr"], fb_level=g["fb_level"], err_max=g["err_max"], **LK, **CORNERS, **kw)


@pytest.mark.parametrize("win,light,gated", [(15, "gain", False), (15, "bias", True), (21, "gain", True), (31, "bias", False)])
def test_pairs_run_is_the_composition_of_stage_entries(pkg, ofk, gpu_ctx, win, light, gated):
    from of_amd.pipeline import FlowPipeline
    B = 4
    prev, nxt, p0 = pairs(B)
    gate = PLAIN_GATE if gated else None
    cfg = config(win, light, gate)
    sensors = ofk.make_sensors(B, d=p0["d"], normal=p0["n"], omega=p0["omega"], scaling=p0["scaling"], cx=p0["cx"], cy=p0["cy"])
    pipe = FlowPipeline(W, H, B, cfg, streams=2)
    try:
        assert pipe.ctx.get_lk_light().mode == ofk.LIGHT_MODES[light] and pipe.ctx.get_lk_light().gain_max == 4.0
        for call in range(2):                                    # the second call runs on the other pyramid set
            pipe.upload(prev, nxt, sensors)
            out = pipe.run()
            # the stage entries on another context: gray, corners, ofk_lk_pyr_light with the gates behind it
            g0 = gpu_ctx.gray_bgr8(prev); g1 = gpu_ctx.gray_bgr8(nxt)
            counts = out["counts"]
            S = int(counts.max())
            stage = gpu_ctx.lk_pyr_fb(g0, g1, out["prev_pts"][:, :S], counts, win=win, light=light, **(gate or G.OFF), **LK)
            fired = 0
            for b in range(B):
                n = int(counts[b]); tag = (win, light, gated, "call", call, "pair", b)
                corners = gpu_ctx.good_features(g0[b], cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size).reshape(-1, 2)
                assert n == len(corners) and np.array_equal(bits(out["prev_pts"][b, :n]), bits(corners)), tag
                for k in ("next_pts", "status", "err"):
                    assert np.array_equal(bits(out[k][b, :n]), bits(stage[k][b, :n])), (tag, k)
                ref = LR.gated_chain(prev[b], nxt[b], cfg, sensors[b], gate or G.OFF, light)
                assert_pair_matches(out, b, ref, str(tag))           # the solve on exactly those points
                fired += int(ref["gate"]["stats"][1] + ref["gate"]["stats"][2])
            if gated:
                assert fired >= 3, fired
    finally:
        pipe.close()


def stream_frames(B, nf):
    from of_amd import synth
    seqs = [synth.render_sequence(H, W, 40 + b, nf, margin=160, **STREAM_MOTION) for b in range(B)]
    frames = np.stack([s[0] for s in seqs]).copy()
    for b in range(B):
        for t in range(1, nf):                                   # auto-exposure hunting: another exposure every frame
            frames[b, t] = synth.apply_exposure(frames[b, t], *EXPOSURES[(t + 2 * b) % len(EXPOSURES)])
    return frames, seqs[0][1]


@pytest.mark.parametrize("kind,light", [("step", "gain"), ("step-gated", "bias"), ("fused-kf3", "gain"), ("step-seeded-gated", "gain")])
def test_stream_steps_under_changing_exposure(pkg, ofk, gpu_ctx, kind, light):
    from of_amd.pipeline import FlowStream, FusionConfig, FilterModel
    nf, B = 5, 2
    gated = kind.endswith("gated")
    seeded = "seeded" in kind
    gate = PLAIN_GATE if gated else dict(G.OFF)
    cfg = config(15, light, gate if gated else None, **(dict(lk_seed="model") if seeded else {}))
    frames, info = stream_frames(B, nf)
    sensors = ofk.make_sensors(B, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"],
                               v_prior=info["v"])
    fusion = FusionConfig(use_imu=False, filter=True, z_sign=1.0, z_source=1, model=FilterModel.kf3()) if kind.startswith("fused") else None
    min_feat, radius = 48, 8
    logs = [[] for _ in range(B)]
    predict = lambda old, src, mode, gain: gpu_ctx.predict_points(np.ascontiguousarray(old, np.float32)[None], np.array([len(old)], np.int32),
                                                                   np.asarray(src, np.float64)[None], mode, gain)[0]
    plug = (dict(lk_src=LR.seeded_gated_lk(cfg, gate, R.SEED_MODEL, light, 1.0, None, predict)) if seeded else {})
    loops = [NodeLoop(frames[b, 0], cfg, min_feat, radius, **(plug if seeded else dict(lk=LR.gated_lk(cfg, gate, light, logs[b]))),
                      **(dict(model=fusion.model) if fusion else {})) for b in range(B)]
    plain = [NodeLoop(frames[b, 0], cfg, min_feat, radius) for b in range(B)]         # the brightness-constancy tracker on the same frames
    first = [l.tracks.copy() for l in loops]
    fs = FlowStream(W, H, batch=B, cfg=cfg, min_features=min_feat, mask_radius=radius, fusion=fusion)
    try:
        tracks, counts = fs.begin(frames[:, 0])
        for b in range(B):
            assert counts[b] == len(first[b]) and np.array_equal(tracks[b, :counts[b]], first[b])
        differs = 0
        for t in range(1, nf):
            if fusion:
                rec, fused, tracks, counts = fs.step_fused(frames[:, t], sensors)
            else:
                rec, tracks, counts = fs.step(frames[:, t], sensors)
            nxt, keep = fs.ctx.stream_last_points(cfg.max_corners)
            for b in range(B):
                o = loops[b].step(frames[b, t], sensors[b]); tag = (kind, light, t, b)
                assert rec[b, 12] == o["n_old"] and rec[b, 13] == o["n_tracked"] and counts[b] == len(o["tracks"]), \
                    (tag, rec[b, 12:14], o["n_old"], o["n_tracked"], counts[b], len(o["tracks"]))
                assert np.array_equal(bits(tracks[b, :counts[b]]), bits(o["tracks"].astype(np.float32))), tag
                assert np.array_equal(keep[b, :o["n_old"]], o["status"]) and np.array_equal(bits(nxt[b, :o["n_old"]]), bits(o["new"])), tag
                if o["v"] is not None:
                    np.testing.assert_allclose(rec[b, :3], o["v"], rtol=1e-8, atol=1e-12, err_msg=str(tag))
                    np.testing.assert_allclose(rec[b, 8:11], o["v_uav"], rtol=1e-8, atol=1e-12, err_msg=str(tag))
                if fusion:
                    np.testing.assert_allclose(fused[b, :3], o["x"], rtol=1e-8, atol=1e-12, err_msg=str(tag))
                if t == 1 and not seeded and not gated:          # same old points on the first step: the light is seen to matter
                    q = plain[b].step(frames[b, t], sensors[b])
                    differs += int(np.sum(bits(q["new"]) != bits(o["new"])))
        if not seeded and not gated:
            assert differs > 20
    finally:
        fs.close()


def test_light_off_after_on_is_the_context_that_never_saw_it(pkg, ofk):
    from of_amd.pipeline import FlowPipeline, FlowStream
    B = 4
    prev, nxt, p0 = pairs(B)
    sensors = ofk.make_sensors(B, d=p0["d"], normal=p0["n"], omega=p0["omega"], scaling=p0["scaling"], cx=p0["cx"], cy=p0["cy"])
    cfg = config(15, None, PLAIN_GATE)
    outs = []
    for touch in (False, True):
        pipe = FlowPipeline(W, H, B, cfg, streams=2)
        try:
            pipe.upload(prev, nxt, sensors)
            if touch:
                pipe.ctx.set_lk_light("gain")
                lit = pipe.run()
                pipe.ctx.set_lk_light(None)
                assert pipe.ctx.get_lk_light().mode == ofk.LIGHT_OFF
            outs.append(pipe.run())
            outs[-1]["gate"] = pipe.ctx.track_gate_download(B)
        finally:
            pipe.close()
    a, b = outs
    for k in ("prev_pts", "next_pts", "status", "err", "counts"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert_records_identical(a["records"], b["records"])
    for k in ("stats", "fb2", "back_pts", "back_status"):
        assert np.array_equal(bits(a["gate"][k]), bits(b["gate"][k])), k
    assert not np.array_equal(bits(lit["next_pts"]), bits(b["next_pts"]))           # and the run in between was a different run
    # the same for a stream
    frames, info = stream_frames(1, 4)
    s1 = ofk.make_sensors(1, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"])
    res = []
    for touch in (False, True):
        fs = FlowStream(W, H, batch=1, cfg=cfg, min_features=48, mask_radius=8)
        try:
            fs.begin(frames[:, 0])
            steps = []
            for t in range(1, 4):
                if touch and t == 1:
                    fs.ctx.set_lk_light("bias", gain_max=2.0)
                    fs.ctx.set_lk_light("off")
                steps.append(fs.step(frames[:, t], s1))
            res.append(steps)
        finally:
            fs.close()
    for (r0, t0, c0), (r1, t1, c1) in zip(*res):
        assert np.array_equal(c0, c1) and np.array_equal(bits(t0), bits(t1)) and np.array_equal(r0.view(np.uint64), r1.view(np.uint64))


def test_exposure_step_end_to_end_on_the_device(pkg, ofk):
    """The "default" row of lk_seed_reference.ROWS, its next BGR frame under (1.25, +10), through ofk_pairs_run.  Measured first on the
    test-side chain on the CPU (tracked / wrong / right / relative error of v): setting off 290 / 145 / 145 / 3.95, bias
    300 / 1 / 299 / 0.0098, gain 300 / 1 / 299 / 0.0090.  The device is held to the bounds of tests/test_lk_light_reference.py."""
    from of_amd import synth
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    e = R.experiment_pair("default"); pair = e["pair"]
    nxt = synth.apply_exposure(pair["next"], 1.25, 10.0)
    sensors = R.experiment_sensors(pair)[None]
    end = e["pts"].astype(np.float64) + e["flow"]
    cfg = PipelineConfig(max_corners=300, quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)
    pipe = FlowPipeline(R.W_EXP, R.H_EXP, 1, cfg)
    try:
        pipe.upload(pair["prev"][None], nxt[None], sensors)
        seen = {}
        for light in (None, "bias", "gain"):
            pipe.ctx.set_lk_light(light)
            out = pipe.run()
            n = int(out["counts"][0])
            assert n == len(e["pts"]) and np.array_equal(out["prev_pts"][0, :n], e["pts"])
            tracked = out["status"][0, :n] == 1
            d = np.linalg.norm(out["next_pts"][0, :n].astype(np.float64) - end, axis=1)
            rel = float(np.linalg.norm(out["records"][0, :3] - pair["v"]) / np.linalg.norm(pair["v"]))
            seen[light] = dict(tracked=int(tracked.sum()), wrong=int((tracked & (d > 0.5)).sum()), right=int((tracked & (d <= 0.5)).sum()), rel=rel)
            print(f"\nlk_light {light}: {seen[light]}")
            ref = LR.gated_chain(pair["prev"], nxt, cfg, sensors[0], G.OFF, light)
            assert_pair_matches(out, 0, ref, str(light))
        assert seen[None]["wrong"] / seen[None]["tracked"] >= 0.30, seen[None]
        for light in ("bias", "gain"):
            r = seen[light]
            assert r["wrong"] <= 3 and r["right"] >= 297 and r["rel"] <= 0.02, (light, r)
    finally:
        pipe.close()
