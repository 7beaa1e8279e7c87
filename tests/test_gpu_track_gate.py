"""GPU: the track gates (ofk_set_track_gate, ofk_lk_pyr_fb) against the test-side reference (tests/track_gate_reference.py).

(1) the stage entry bit for bit over the LK kernel routes and the three backward-pass variants, ragged counts and an empty image;
(2) ofk_pairs_run over slice counts and overlap settings, four consecutive upload + run calls on alternating pyramid sets;
(3) FlowStream.step / step_fused / the robust solve against the restated stream loop with the gated tracker;
(4) off means off; (5) refusals.
Every case first asserts on the reference that the gate fires: a test in which it never does proves nothing."""
import numpy as np
import pytest

from oracle import image_oracle as io
import lk_seed_reference as R  # noqa: E402  (tests/lk_seed_reference.py)
import track_gate_reference as G  # noqa: E402  (tests/track_gate_reference.py)
from batch_oracle import assert_pair_matches  # noqa: E402  (tests/batch_oracle.py)
from stream_oracle import NodeLoop  # noqa: E402  (tests/stream_oracle.py)

pytestmark = pytest.mark.gpu

H, W = 240, 320
MOTION = dict(v=(0.003, -0.002, 0.001), omega=(0.03, -0.02, 0.1))
LK = dict(max_level=2, max_count=20, eps=0.03, min_eig_thr=1e-4)
CORNERS = dict(max_corners=60, quality=0.01, min_distance=5, block_size=5)
VARIANTS = {"plain-L2": dict(fb="plain", fb_level=2), "seeded-L2": dict(fb="seeded", fb_level=2), "seeded-L0": dict(fb="seeded", fb_level=0)}
_scenes, _chains = {}, {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def scene(seed=5):
    if seed not in _scenes:
        from of_amd import synth
        pair = synth.render_pair(H, W, seed, margin=64, **MOTION)
        g0, g1 = io.gray_bgr8(pair["prev"]), io.gray_bgr8(pair["next"])
        pts = io.good_features(g0, CORNERS["max_corners"], CORNERS["quality"], CORNERS["min_distance"], CORNERS["block_size"]).reshape(-1, 2)
        _scenes[seed] = dict(pair=pair, g0=g0, g1=g1, pts=pts)
    return _scenes[seed]


def assert_gate_fires(r, tag):
    assert r["stats"][2] >= 5 and int(r["keep"].sum()) >= 20, (tag, r["stats"], int(r["keep"].sum()))


# window, variant, forward seed, err cap
STAGE = [pytest.param(win, var, False, False, id=f"win{win}-{var}") for win in (5, 15, 21, 31) for var in VARIANTS]
STAGE += [pytest.param(15, "seeded-L2", True, False, id="win15-seeded-L2-forward-seeded"), pytest.param(21, "plain-L2", True, False, id="win21-plain-L2-forward-seeded"),
          pytest.param(15, "plain-L2", False, True, id="win15-plain-L2-errcap"), pytest.param(31, "seeded-L0", False, True, id="win31-seeded-L0-errcap")]


@pytest.mark.parametrize("win,var,fseed,cap", STAGE)
def test_stage_entry_bit_for_bit(pkg, ofk, gpu_ctx, win, var, fseed, cap):
    s = scene()
    n = len(s["pts"])
    counts = np.array([n, min(37, n), 1, 0], np.int32)           # a ragged tail for the four-points-per-wave kernel and an empty image
    gate = G.setting(fb_thr=0.5, **VARIANTS[var])
    if cap:                                                      # the median err of the tracked points: about half of them fall to it
        base = G.gated(s["g0"], s["g1"], s["pts"], win, gate=G.OFF, **LK)
        gate["err_max"] = float(np.median(base["err"][base["st_f"] == 1]))
    seed = (s["pts"] + np.array([3, -2], np.float32)).astype(np.float32) if fseed else None
    flags = R.USE_INITIAL_FLOW if fseed else 0
    refs = [G.gated(s["g0"], s["g1"], s["pts"][:c], win, gate=gate, seed=None if seed is None else seed[:c], flags=flags, **LK) for c in counts]
    assert_gate_fires(refs[0], (win, var))
    if cap:
        assert refs[0]["stats"][3] >= 5, refs[0]["stats"]
    B = len(counts)
    prev = np.repeat(s["g0"][None], B, 0); nxt = np.repeat(s["g1"][None], B, 0)
    pp = np.repeat(s["pts"][None], B, 0)
    out = gpu_ctx.lk_pyr_fb(prev, nxt, pp, counts, win=win, next_pts=None if seed is None else np.repeat(seed[None], B, 0), flags=flags,
                            **gate, **LK)
    assert gpu_ctx.get_track_gate().fb_mode == ofk.FB_OFF
    dl = gpu_ctx.track_gate_download(B)                          # the stage entry took its own setting: the context's stays off
    for b, (c, r) in enumerate(zip(counts, refs)):
        tag = (win, var, "image", b)
        assert np.array_equal(bits(out["next_pts"][b, :c]), bits(r["next"])), tag
        assert np.array_equal(out["status"][b, :c], r["status"]), tag
        assert np.array_equal(bits(out["err"][b, :c]), bits(r["err"])), tag
        assert np.array_equal(bits(out["back_pts"][b, :c]), bits(r["back"])), tag
        assert np.array_equal(out["back_status"][b, :c], r["st_b"]), tag
        assert np.array_equal(bits(out["fb2"][b, :c]), bits(r["fb2"])), tag
        assert np.array_equal(dl["stats"][b], r["stats"]), (tag, dl["stats"][b], r["stats"])
        assert np.array_equal(bits(dl["fb2"][b, :c]), bits(r["fb2"])) and np.array_equal(bits(dl["back_pts"][b, :c]), bits(r["back"])), tag


def pairs_cfg(win, var):
    from of_amd.pipeline import PipelineConfig
    g = VARIANTS[var]
    return PipelineConfig(win=win, max_level=LK["max_level"], max_count=LK["max_count"], eps=LK["eps"], min_eig_thr=LK["min_eig_thr"],
                          fb_check=g["fb"], fb_thr=0.5, fb_level=g["fb_level"], **CORNERS)


def pair_sensors(ofk, B):
    p = scene(5)["pair"]
    return ofk.make_sensors(B, d=p["d"], normal=p["n"], omega=p["omega"], scaling=p["scaling"], cx=p["cx"], cy=p["cy"])


def chain(seed, win, var, sensors_row):
    key = (seed, win, var)
    if key not in _chains:
        cfg = pairs_cfg(win, var)
        p = scene(seed)["pair"]
        _chains[key] = G.gated_chain(p["prev"], p["next"], cfg, sensors_row, G.setting(fb_thr=0.5, **VARIANTS[var]))
    return _chains[key]


@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "serial"])
@pytest.mark.parametrize("slices", [1, 2])
@pytest.mark.parametrize("var", ["seeded-L0", "plain-L2"])
@pytest.mark.parametrize("win", [15, 21])
def test_pairs_run_gated(pkg, ofk, win, var, slices, overlap):
    from of_amd.pipeline import FlowPipeline
    seeds = (5, 6, 7, 8)
    B = len(seeds)
    sensors = pair_sensors(ofk, B)
    cfg = pairs_cfg(win, var)
    refs = {sd: chain(sd, win, var, sensors[0]) for sd in seeds}
    for sd in seeds:
        assert_gate_fires(refs[sd]["gate"], (win, var, sd))
    pipe = FlowPipeline(W, H, B, cfg, streams=slices)
    try:
        pipe.ctx.set_overlap(overlap)
        g = pipe.ctx.get_track_gate()
        assert (g.fb_mode, g.fb_thr, g.fb_level, g.err_max) == (ofk.FB_MODES[VARIANTS[var]["fb"]], 0.5, VARIANTS[var]["fb_level"], 0.0)
        for call in range(4):                                    # the two pyramid sets alternate: each is rewritten twice
            order = [seeds[(b + call) % B] for b in range(B)]
            prev = np.stack([scene(sd)["pair"]["prev"] for sd in order]); nxt = np.stack([scene(sd)["pair"]["next"] for sd in order])
            pipe.upload(prev, nxt, sensors)
            out = pipe.run()
            dl = pipe.ctx.track_gate_download(B)
            assert np.array_equal(pipe.track_gate_stats(), dl["stats"])
            for b, sd in enumerate(order):
                ref = refs[sd]; r = ref["gate"]; n = len(ref["pts"]); tag = (win, var, slices, overlap, "call", call, "pair", b)
                assert_pair_matches(out, b, ref, str(tag))
                assert np.array_equal(dl["stats"][b], r["stats"]), (tag, dl["stats"][b], r["stats"])
                assert np.array_equal(bits(dl["fb2"][b, :n]), bits(r["fb2"])) and np.array_equal(bits(dl["back_pts"][b, :n]), bits(r["back"])), tag
                assert np.array_equal(dl["back_status"][b, :n], r["st_b"]), tag
    finally:
        pipe.close()


STREAM_MOTION = dict(v=(0.003, -0.002, 0.001), omega=(0.015, -0.01, 0.05), d=1.0)      # half the pair's rotation per frame


@pytest.mark.parametrize("kind,var", [("step", "seeded-L0"), ("step", "plain-L2"), ("fused-kf3", "seeded-L2"), ("robust", "seeded-L0")])
def test_stream_steps_gated(pkg, ofk, kind, var):
    from of_amd import synth
    from of_amd.pipeline import FlowStream, FusionConfig, FilterModel
    import robust_stream_oracle as rso
    nf, B = 6, 2
    cfg = pairs_cfg(15, var)
    if kind == "robust":
        cfg.robust = "tukey"; cfg.robust_c = rso.SETTING["c"]; cfg.robust_iters = rso.SETTING["iters"]
        cfg.robust_hypotheses = rso.SETTING["hypotheses"]; cfg.robust_seed = rso.SETTING["seed"]
    gate = G.setting(fb_thr=0.5, **VARIANTS[var])
    seqs = [synth.render_sequence(H, W, 40 + b, nf, margin=160, **STREAM_MOTION) for b in range(B)]
    frames = np.stack([s[0] for s in seqs]); info = seqs[0][1]
    sensors = ofk.make_sensors(B, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"])
    fusion = FusionConfig(use_imu=False, filter=True, z_sign=1.0, z_source=1, model=FilterModel.kf3()) if kind == "fused-kf3" else None
    min_feat, radius = 48, 8                                     # the reference re-detects in both streams (46 tracks before the last step)
    # the reference first: the comparison below means something only if the gate removes tracks and a stream re-detects
    logs = [[] for _ in range(B)]
    loops = [NodeLoop(frames[b, 0], cfg, min_feat, radius, lk=G.gated_lk(cfg, gate, logs[b]),
                      **(dict(solve=rso.robust_solver(b, False, False)) if kind == "robust" else {}),
                      **(dict(model=fusion.model) if fusion else {})) for b in range(B)]
    first = [l.tracks.copy() for l in loops]
    ref = [[loops[b].step(frames[b, t], sensors[b]) for b in range(B)] for t in range(1, nf)]
    pruned = sum(int(r["stats"][1] + r["stats"][2]) for lg in logs for r in lg)
    redetected = sum(int(len(o["tracks"]) > o["n_tracked"]) for row in ref for o in row)
    assert pruned >= 5 and redetected >= 1, (pruned, redetected)
    fs = FlowStream(W, H, batch=B, cfg=cfg, min_features=min_feat, mask_radius=radius, fusion=fusion)
    try:
        tracks, counts = fs.begin(frames[:, 0])
        for b in range(B):
            assert counts[b] == len(first[b]) and np.array_equal(tracks[b, :counts[b]], first[b])
        for t in range(1, nf):
            if fusion:
                rec, fused, tracks, counts = fs.step_fused(frames[:, t], sensors)
            else:
                rec, tracks, counts = fs.step(frames[:, t], sensors)
            stats = fs.track_gate_stats()
            nxt, keep = fs.ctx.stream_last_points(cfg.max_corners)
            for b in range(B):
                o = ref[t - 1][b]; r = logs[b][t - 1]; tag = (kind, var, t, b)
                assert rec[b, 12] == o["n_old"] and rec[b, 13] == o["n_tracked"] and counts[b] == len(o["tracks"]), \
                    (tag, rec[b, 12:14], o["n_old"], o["n_tracked"], counts[b], len(o["tracks"]))
                assert np.array_equal(bits(tracks[b, :counts[b]]), bits(o["tracks"].astype(np.float32))), tag
                assert np.array_equal(stats[b], r["stats"]), (tag, stats[b], r["stats"])
                assert np.array_equal(keep[b, :o["n_old"]], r["status"]) and np.array_equal(bits(nxt[b, :o["n_old"]]), bits(r["next"])), tag
                if o["v"] is not None:
                    np.testing.assert_allclose(rec[b, :3], o["v"], rtol=1e-8, atol=1e-12, err_msg=str(tag))
                    np.testing.assert_allclose(rec[b, 8:11], o["v_uav"], rtol=1e-8, atol=1e-12, err_msg=str(tag))
                if fusion:
                    np.testing.assert_allclose(fused[b, :3], o["x"], rtol=1e-8, atol=1e-12, err_msg=str(tag))
    finally:
        fs.close()


def test_download_returns_the_rows_asked_for(pkg, ofk):
    """The library writes the rows of the latest gated run, whatever the caller asks for: the binding's buffers must hold them all,
    and a download of fewer rows, of none, or of the counts alone returns just that."""
    s = scene()
    n = len(s["pts"])
    B = 4
    gate = G.setting(fb_thr=0.5, **VARIANTS["seeded-L0"])
    r = G.gated(s["g0"], s["g1"], s["pts"], 15, gate=gate, **LK)
    assert_gate_fires(r, "download")
    ctx = ofk.Context(0, W, H, B, n, LK["max_level"])
    try:
        ctx.lk_pyr_fb(np.repeat(s["g0"][None], B, 0), np.repeat(s["g1"][None], B, 0), np.repeat(s["pts"][None], B, 0), [n] * B, win=15, **gate, **LK)
        for rows in (1, 2, 0, B):
            dl = ctx.track_gate_download(rows)
            assert dl["stats"].shape == (rows, 4) and dl["fb2"].shape == (rows, n) and dl["back_pts"].shape == (rows, n, 2) and dl["back_status"].shape == (rows, n)
            for b in range(rows):
                assert np.array_equal(dl["stats"][b], r["stats"]) and np.array_equal(bits(dl["fb2"][b]), bits(r["fb2"]))
                assert np.array_equal(bits(dl["back_pts"][b]), bits(r["back"])) and np.array_equal(dl["back_status"][b], r["st_b"])
            only = ctx.track_gate_download(rows, points=False)
            assert set(only) == {"stats"} and np.array_equal(only["stats"], dl["stats"]) and np.array_equal(ctx.track_gate_stats(rows), dl["stats"])
        with pytest.raises(ValueError):
            ctx.track_gate_download(B + 1)
        cap = dict(gate, fb="off", err_max=float(np.median(r["err"][r["st_f"] == 1])))      # the err cap alone: no backward pass, zeros
        ctx.lk_pyr_fb(s["g0"][None], s["g1"][None], s["pts"][None], [n], win=15, **cap, **LK)
        dl = ctx.track_gate_download(1)
        assert dl["stats"][0, 3] >= 5 and not dl["fb2"].any() and not dl["back_pts"].any() and not dl["back_status"].any()
    finally:
        ctx.close()


def test_off_means_off(pkg, ofk):
    from of_amd import synth
    from of_amd.pipeline import FlowPipeline, FlowStream
    B = 4
    cfg = pairs_cfg(15, "seeded-L0"); cfg.fb_check = "off"
    sensors = pair_sensors(ofk, B)
    prev = np.stack([scene(sd)["pair"]["prev"] for sd in (5, 6, 7, 8)]); nxt = np.stack([scene(sd)["pair"]["next"] for sd in (5, 6, 7, 8)])
    frames, info = synth.render_sequence(H, W, 40, 4, margin=160, **STREAM_MOTION)
    s1 = ofk.make_sensors(1, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"])

    def touch(ctx, how):
        if how == "set-and-cleared":
            ctx.set_track_gate(fb="seeded", fb_thr=0.5, fb_level=0, err_max=5.0)
            ctx.set_track_gate(None)
        elif how == "explicit-off":
            ctx.set_track_gate(fb="off", err_max=0.0)
        g = ctx.get_track_gate()
        assert g.fb_mode == ofk.FB_OFF and g.err_max == 0.0

    pairs, streams = [], []
    for how in ("never", "set-and-cleared", "explicit-off", "cleared-after-a-gated-run"):
        pipe = FlowPipeline(W, H, B, cfg, streams=2)
        try:
            pipe.upload(prev, nxt, sensors)
            touch(pipe.ctx, how)
            if how == "cleared-after-a-gated-run":               # a gated run in between leaves nothing behind
                pipe.ctx.set_track_gate(fb="plain", fb_thr=0.5)
                gated = pipe.run()
                pipe.ctx.set_track_gate(None)
            pairs.append(pipe.run())
        finally:
            pipe.close()
        fs = FlowStream(W, H, batch=1, cfg=cfg, min_features=45, mask_radius=8)
        try:
            if how == "cleared-after-a-gated-run":               # the stream is begun anew behind a gated step
                fs.begin(frames[None, 0])
                fs.ctx.set_track_gate(fb="seeded", fb_thr=0.5, fb_level=0)
                fs.step(frames[None, 1], s1)
                assert fs.track_gate_stats()[0, 0] > 0
                fs.ctx.set_track_gate(None)
            fs.begin(frames[None, 0])
            touch(fs.ctx, how)
            steps = [fs.step(frames[None, t], s1) for t in range(1, 4)]
            streams.append(steps)
        finally:
            fs.close()
    for other in pairs[1:]:
        for k in ("prev_pts", "next_pts", "status", "err", "counts"):
            assert np.array_equal(bits(pairs[0][k]), bits(other[k])), k
        assert np.array_equal(pairs[0]["records"].view(np.uint64), other["records"].view(np.uint64))
    assert not np.array_equal(gated["status"], pairs[0]["status"])       # and the gated run in between was a different run
    for other in streams[1:]:
        for (r0, t0, c0), (r1, t1, c1) in zip(streams[0], other):
            assert np.array_equal(c0, c1) and np.array_equal(bits(t0), bits(t1)) and np.array_equal(r0.view(np.uint64), r1.view(np.uint64))


def test_refusals(pkg, ofk):
    from of_amd.pipeline import FlowPipeline
    B = 2
    cfg = pairs_cfg(15, "seeded-L0")
    sensors = pair_sensors(ofk, B)
    s = scene()
    prev = np.stack([scene(sd)["pair"]["prev"] for sd in (5, 6)]); nxt = np.stack([scene(sd)["pair"]["next"] for sd in (5, 6)])
    pipe = FlowPipeline(W, H, B, cfg)
    try:
        ctx = pipe.ctx
        pipe.upload(prev, nxt, sensors)
        want = pipe.run()
        before = ctx.get_track_gate()
        fresh = ofk.Context(0, W, H, 1, 60, 2)
        try:
            with pytest.raises(ofk.OfkError, match="no run or step"):    # nothing to download before a gated run
                fresh.track_gate_download(1)
        finally:
            fresh.close()
        TG = ofk.TrackGate
        for bad, word in ((TG(3, 0.5, -1, 0.0), "fb_mode"), (TG(-1, 0.5, -1, 0.0), "fb_mode"), (TG(1, 0.0, -1, 0.0), "fb_thr"),
                          (TG(2, -0.5, -1, 0.0), "fb_thr"), (TG(1, float("nan"), -1, 0.0), "fb_thr"), (TG(1, float("inf"), -1, 0.0), "fb_thr"),
                          (TG(1, 0.5, -2, 0.0), "fb_level"), (TG(1, 0.5, cfg.max_level + 1, 0.0), "fb_level"), (TG(0, 0.5, -1, -1.0), "err_max"),
                          (TG(0, 0.5, -1, float("nan")), "err_max"), (TG(1, 0.5, -1, float("inf")), "err_max")):
            with pytest.raises(ofk.OfkError, match=word) as e:
                ctx.set_track_gate(bad)
            assert e.value.code == ofk.E_INVALID
            now = ctx.get_track_gate()                                   # the previous setting stays in place
            assert (now.fb_mode, now.fb_thr, now.fb_level, now.err_max) == (before.fb_mode, before.fb_thr, before.fb_level, before.err_max)
            with pytest.raises(ofk.OfkError, match=word) as e:           # the stage entry refuses the same settings before any launch
                ctx.lk_pyr_fb(s["g0"][None], s["g1"][None], s["pts"][None], [len(s["pts"])], gate=bad, **LK)
            assert e.value.code == ofk.E_INVALID
        for bad in (TG(0, 0.5, -2, 0.0), TG(0, 0.5, 99, 0.0)):           # nothing switched on, and still no valid setting
            for call in (lambda: ctx.set_track_gate(bad),
                         lambda: ctx.lk_pyr_fb(s["g0"][None], s["g1"][None], s["pts"][None], [len(s["pts"])], gate=bad, **LK)):
                with pytest.raises(ofk.OfkError, match="fb_level") as e:
                    call()
                assert e.value.code == ofk.E_INVALID
        off = ctx.lk_pyr_fb(s["g0"][None], s["g1"][None], s["pts"][None], [len(s["pts"])], gate=TG(0, 0.5, -1, 0.0), **LK)     # a valid "off" is ofk_lk_pyr_ex
        plain = ctx.lk_pyr(s["g0"][None], s["g1"][None], s["pts"][None], [len(s["pts"])], **LK)
        assert np.array_equal(bits(off["next_pts"]), bits(plain[0])) and np.array_equal(off["status"], plain[1]) and np.array_equal(bits(off["err"]), bits(plain[2]))
        with pytest.raises(ofk.OfkError, match="GET_MIN_EIGENVALS") as e:
            ctx.lk_pyr_fb(s["g0"][None], s["g1"][None], s["pts"][None], [len(s["pts"])], fb="plain", err_max=4.0, flags=ofk.LK_GET_MIN_EIGENVALS, **LK)
        assert e.value.code == ofk.E_INVALID
        pipe.upload(prev, nxt, sensors)                                  # the stage entry used the frame buffers
        again = pipe.run()
        for k in ("prev_pts", "next_pts", "status", "err", "counts"):
            assert np.array_equal(bits(want[k]), bits(again[k])), k
        assert np.array_equal(want["records"].view(np.uint64), again["records"].view(np.uint64))
    finally:
        pipe.close()
