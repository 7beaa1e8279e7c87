"""GPU: stream and pair runs with several settings switched on at once (seeded LK, track gates, corner grid, robust solve with drop,
velocity covariance, exclusion zones) against the composed reference of tests/combined_cases.py, step by step.  Each setting's own
suite shows "off is bit-identical" and "on, alone, equals the reference"; here the host functions that every setting added lines to
(stream_step_impl, track, solve_pairs, ofk_pairs_run) run with the settings together, as a deployed stream does.

(a) everything on in the fused step on the resident IMU state with the 6-state filter corrected by the covariance kernel
(b) the same on the plain step (the covariance comes from the pairs kernel inside a stream step)
(c) pairs of settings on the plain step; gate + zones: a point the gate refused is lost, not a reject (zones rule 1)
(d) the other two sources of rejects: the feasibility rule, and the legacy keep with the replacing detection through the grid
(e) a held step leaves the zone table untouched, its age included      (f) ofk_stream_begin clears the table
(g) frame pairs in both launch forms; ofk_pairs_run ignores the zones setting
(h) all six set and switched off again before begin == never set

Comparison rules are the suite's: tracks, counts, zone tables, gate and grid statistics bit for bit; velocity rtol 1e-8 / atol 1e-12
(tests/test_gpu_zones.py); covariance records within tests/test_gpu_cov.py's 1e-9 bound, fed - as there - with the device's own
record and weights; filter x and P rtol 1e-9.  tests/test_combined_reference.py shows on the CPU that every reference run is active
in every setting and free of near-ties, and that the wrong references of (c) and (e) differ in what is asserted here."""
import numpy as np
import pytest

import combined_cases as cc
import cov_reference as cr
from point_stage_helpers import bits

pytestmark = pytest.mark.gpu

H, W, NB = cc.H, cc.W, cc.NB
_cache = {}


def assert_cov_close(got, ref, tag):
    from test_gpu_cov import assert_cov_close as close          # tests/test_gpu_cov.py: the 1e-9 bound and its reasoning
    close(got, ref, tag)


@pytest.fixture(scope="module")
def scene(pkg, ofk):
    from of_amd import synth
    frames, info = cc.sequences(synth)
    return frames, info, cc.sensor_rows(ofk, info)


def device_predict(ctx):
    """The seed predictor of the reference's tracker plug: ofk_predict_points (a stage entry, on another context than the stream's).
    It agrees with lk_seed_reference.predict to an ulp (tests/test_gpu_seed_pipeline.py); LK's bits follow the seed's."""
    def predict(old, src, mode, gain):
        p = np.ascontiguousarray(old, np.float32).reshape(1, -1, 2)
        return ctx.predict_points(p, np.array([p.shape[1]], np.int32), np.asarray(src, np.float64)[None], mode, gain)[0]
    return predict


def assert_zones_equal(got, b, z, tag):
    assert np.array_equal(got["stats"][b], z.stats), (tag, got["stats"][b], z.stats)
    assert np.array_equal(got["zones"][b], z.zones) and np.array_equal(bits(got["motion"][b]), bits(z.motion)), (tag, got["zones"][b][:, :9], z.zones[:, :9])


def run_stream_case(ofk, gpu_ctx, scene, name, nf=cc.NF, on_step=None):
    """The case on the device against its reference, every step of every stream; returns the reference (its counters filled)."""
    from of_amd.pipeline import FlowStream, PipelineConfig, FusionConfig
    frames, info, sr = scene
    ref = cc.Reference(name, PipelineConfig, frames, info, sr, predict=device_predict(gpu_ctx))
    cfg, kind = ref.cfg, ref.kind
    fusion = None if kind == "step" else FusionConfig(use_imu=False) if kind == "fused" else FusionConfig.ekf6(**cc.EKF)
    fs = FlowStream(W, H, batch=NB, cfg=cfg, min_features=cc.MIN_FEAT, mask_radius=cc.RADIUS, fusion=fusion)
    try:
        if kind == "ekf6":
            fs.ctx.imu_reset(NB, cc.imu_state0(info))
        tracks, counts = fs.begin(frames[:, 0])
        for b in range(NB):
            assert counts[b] == len(ref.loops[b].tracks) and np.array_equal(bits(tracks[b, :counts[b]]), bits(ref.loops[b].tracks)), (name, b)
        if ref.grid_on:
            st = fs.corner_grid_stats()
            assert [tuple(int(v) for v in st[b]) for b in range(NB)] == [ref.first_grid[b][0] for b in range(NB)]
        for t in range(1, nf):
            msgs, srcs, imu, dv = [()] * NB, [None] * NB, [None] * NB, [None] * NB
            if kind == "ekf6":
                msgs = cc.imu_batch(t)
                fs.push_imu(msgs)
                imu, dv = fs.ctx.imu_state(NB)                   # what the step reads: velocity 0..2, rotation 6..14, normal 15..17, omega 18..20
                srcs = sr.copy(); srcs[:, 1:4] = imu[:, 15:18]; srcs[:, 4:7] = imu[:, 18:21]; srcs[:, 22:25] = imu[:, 0:3]
            if kind == "step":
                rec, tracks, counts = fs.step(frames[:, t], sr)
                fused = None
            else:
                rec, fused, tracks, counts = fs.step_fused(frames[:, t], sr)
            nxt, keep = fs.ctx.stream_last_points(cfg.max_corners)
            zones = fs.zones() if ref.zones_on else None
            gstats = fs.track_gate_stats() if ref.gated else None
            grid = fs.corner_grid_stats() if ref.grid_on else None
            wts, rst = fs.ctx.robust_download(NB) if ref.robust_on else (None, None)
            cov = fs.covariances() if ref.cov_on else None
            fx, fP = fs.ctx.filter_state(NB) if ref.filters is not None else (None, None)
            for b in range(NB):
                o = ref.step(t, b, msgs[b], src=srcs[b])
                tag = (name, t, b)
                n = o["n_old"]
                assert rec[b, 12] == n and rec[b, 13] == o["n_tracked"] and rec[b, 11] == o["used"] and counts[b] == len(o["tracks"]), \
                    (tag, rec[b, 11:14], n, o["n_tracked"], o["used"], counts[b], len(o["tracks"]))
                assert np.array_equal(bits(nxt[b, :n]), bits(o["new"])) and np.array_equal(keep[b, :n], np.asarray(o["keep"]).astype(np.uint8)), tag
                assert np.array_equal(bits(tracks[b, :counts[b]]), bits(o["tracks"].astype(np.float32))), tag
                np.testing.assert_allclose(rec[b, :3], o["v"], rtol=1e-8, atol=1e-12, err_msg=str(tag))
                np.testing.assert_allclose(rec[b, 8:11], o["v_uav"], rtol=1e-8, atol=1e-12, err_msg=str(tag))
                if kind != "step":
                    assert rec[b, 15] == 1 and fused[b, 7] == 1, tag
                if ref.gated:
                    assert np.array_equal(gstats[b], o["gate"]["stats"]), (tag, gstats[b], o["gate"]["stats"])
                if ref.grid_on and o["grid"] is not None:
                    assert tuple(int(v) for v in grid[b]) == tuple(o["grid"]), (tag, grid[b], o["grid"])
                if ref.robust_on:
                    np.testing.assert_array_equal(rst[b, [3, 4, 6, 7]], o["stats"][[3, 4, 6, 7]], err_msg=str(tag))
                    np.testing.assert_allclose(wts[b, :n], o["weights"], rtol=0, atol=1e-9, err_msg=str(tag))
                if ref.zones_on:
                    assert_zones_equal(zones, b, o["zones"], tag)
                if ref.cov_on:
                    # the reference's points, keep flags and motion source; v, RSS, rank, the weights and the control are the device's own, as in test_gpu_cov.py
                    cv, x, P, fz = ref.cov_record(b, o, rec=rec[b], weights=None if wts is None else wts[b, :n], imu=imu[b], control=dv[b])
                    assert cv[13] == 0, tag
                    kept = np.asarray(o["keep"], bool)
                    R_, nrm, om, _ = o["motion"]
                    assert cr.condition(cr.NODE, o["old"], o["new"], kept, sr[b], nrm=nrm, omega=om, w=None if wts is None else wts[b, :n]) < 1e3, tag
                    assert_cov_close(cov[b], cv, str(tag))
                    if ref.filters is not None:
                        assert cov[b, 15] == cv[15] and abs(cov[b, 14] - cv[14]) <= 1e-9 * cv[14] and cv[14] > 0, (tag, cov[b, 14:16], cv[14:16])
                        np.testing.assert_allclose(fx[b], x, rtol=1e-9, atol=1e-15, err_msg=str(tag))
                        np.testing.assert_allclose(fP[b], P, rtol=1e-9, atol=1e-18, err_msg=str(tag))
                        np.testing.assert_allclose(fused[b], fz, rtol=1e-9, atol=1e-15, err_msg=str(tag))
                    else:
                        assert cov[b, 14] == 0 and cov[b, 15] == 0, tag
                if on_step is not None:
                    on_step(t, b, o, zones)
        c = ref.counters
        print(f"{name}: zones inserted {c['inserted']}, refreshed {c['refreshed']}, re-detections behind a zone mask {c['masked']}, gate-refused {c['refused']} "
              f"(steps with rejects too: {c['refused_with_rejects']}), dropped {c['dropped']}, grid examined/accepted {c['examined']}/{c['accepted']} "
              f"(bound in {c['grid_bound']} re-detections), NIS-gated steps {c['nis_gated']} of {c['nis_steps']}, cov records {c['cov_records']}")
        assert c["solved"] == (nf - 1) * NB
        assert not ref.zones_on or (c["inserted"] > 0 and c["masked"] > 0)
        assert not ref.gated or c["refused"] > 0
        assert not ref.grid_on or c["grid_bound"] > 0
        assert not (ref.robust_on or cfg.use_feasibility) or c["dropped"] > 0
        assert not ref.cov_on or c["cov_records"] == c["solved"]
        assert ref.filters is None or 0 < c["nis_gated"] < c["nis_steps"]
        return ref
    finally:
        fs.close()


def test_everything_on_fused(pkg, ofk, gpu_ctx, scene):
    """(a) ekf6 with pushed IMU messages, seed "model" from the resident state, seeded backward pass on level 0 + err cap, binding grid,
    Tukey with drop, propagate with cov_filter, r_floor and a NIS gate that closes on some steps, zones."""
    ref = run_stream_case(ofk, gpu_ctx, scene, "all-fused")
    assert ref.counters["refused_with_rejects"] > 0 and ref.counters["seeded"] == ref.counters["solved"]


def test_everything_on_plain_step(pkg, ofk, gpu_ctx, scene):
    """(b) no filter: solve_pairs' robust kernel clears the dropped points' status, the pairs covariance kernel reads it behind."""
    run_stream_case(ofk, gpu_ctx, scene, "all-step")


def test_covariance_does_not_see_whether_the_point_was_dropped(pkg, ofk, scene):
    """ofk.h, ofk_set_cov: a point the robust drop removes has weight 0 and a cleared keep flag when the covariance kernel runs: the
    step's cov record (and result record) is the same with drop 0 and drop 1, on the plain step and on the fused one."""
    from of_amd.pipeline import FlowStream, PipelineConfig, FusionConfig
    frames, info, sr = scene
    for fused in (False, True):
        got = []
        for drop in (False, True):
            cfg = PipelineConfig(**dict(cc.CASES["all-step"]["cfg"], robust_drop=drop))
            fs = FlowStream(W, H, batch=NB, cfg=cfg, min_features=cc.MIN_FEAT, mask_radius=cc.RADIUS, fusion=FusionConfig(use_imu=False) if fused else None)
            try:
                fs.begin(frames[:, 0])
                out = fs.step_fused(frames[:, 1], sr) if fused else fs.step(frames[:, 1], sr)
                nxt, keep = fs.ctx.stream_last_points(cfg.max_corners)
                got.append((out[0], fs.covariances(), fs.ctx.robust_download(NB)[0], keep, out[-1]))
            finally:
                fs.close()
        (r0, c0, w0, k0, n0), (r1, c1, w1, k1, n1) = got
        assert np.array_equal(bits(r0), bits(r1)) and np.array_equal(bits(c0), bits(c1)) and np.array_equal(bits(w0), bits(w1)), fused
        dropped = int(np.count_nonzero(k0 != k1))
        print(f"fused {fused}: points the drop removed {dropped}, tracks {n0.tolist()} -> {n1.tolist()}")
        assert dropped > 0 and np.all(c0[:, 13] == 0) and np.all(n1 < n0)


@pytest.mark.parametrize("name", ["grid-zones", "gate-zones", "seed-gate-robust"])
def test_pairs_of_settings_on_the_plain_step(pkg, ofk, gpu_ctx, scene, name):
    """(c) grid + zones: occupancy list and zone mask in one append-mode detection; gate + zones; seed + gate + robust."""
    seen = []

    def rule_1(t, b, o, zones):
        # Zones rule 1: "status behind the track gates".  On the first step both streams have points the gate refused with forward status
        # 1 and rejects of the robust drop; the device's count of rejects is the reference's, which leaves the refused points out.  A
        # device that copied the status ahead of the gate would count them (test_combined_reference.py: that reference differs here).
        if t == 1:
            g, kept = o["gate"], np.asarray(o["keep"], bool)
            rejects = int(np.count_nonzero((g["status"] == 1) & ~kept)); ahead = int(np.count_nonzero((g["st_f"] == 1) & ~kept))
            assert o["refused"] > 0 and 0 < rejects < ahead, (b, rejects, ahead)
            assert zones["stats"][b, 4] == rejects == o["zones"].stats[4], (b, zones["stats"][b], rejects, ahead)
            seen.append((rejects, ahead))
    run_stream_case(ofk, gpu_ctx, scene, name, on_step=rule_1 if name == "gate-zones" else None)
    if name == "gate-zones":
        print("gate-zones, first step (rejects seen, tracked-ahead-of-the-gate and not kept):", seen)
        assert len(seen) == NB


def test_feasibility_rule_feeds_the_zones(pkg, ofk, gpu_ctx, scene):
    """(d) the robust solve off: the rejects are the tracked points with r_tilde > feas_T, node-style fused step on the sensors."""
    ref = run_stream_case(ofk, gpu_ctx, scene, "feasibility")
    assert not ref.robust_on and ref.counters["rejects"] == ref.counters["dropped"] > 0


def of_module_stream(ofk, frames, cfg, inp, nb, hold=False):
    from of_amd.pipeline import FlowStream, FusionConfig
    fusion = FusionConfig.of_module(synthetic_flow=False, hold_on_skip=hold)
    return FlowStream(W, H, batch=nb, cfg=cfg, min_features=cc.OFM_MIN_FEAT, mask_radius=10, fusion=fusion), fusion


def of_module_sensors(ofk, inp, t, nb):
    s = np.concatenate([ofk.make_sensors(1, d=1.0, normal=inp["normal"], omega=inp["omegas"][t - 1, b], scaling=1.0, cx=inp["cx"], cy=inp["cy"]) for b in range(nb)])
    s[:, 25:28] = inp["controls"][t - 1]
    return s


def assert_of_module_step(rec, fused, tracks, counts, fx, fP, b, s, tag):
    v, xk, P, tr, n_old, n_keep = s[:6]
    assert rec[b, 12] == n_old and rec[b, 11] == n_keep and counts[b] == len(tr), (tag, rec[b, 11:14], n_old, n_keep, len(tr))
    assert np.array_equal(bits(tracks[b, :counts[b]]), bits(tr.astype(np.float32))), tag
    if v is None:
        assert rec[b, 15] == 0 and fused[b, 7] == 0, tag
    else:
        assert rec[b, 15] == 1 and fused[b, 7] == 1, tag
        np.testing.assert_allclose(rec[b, :3], v, rtol=1e-8, atol=1e-12, err_msg=str(tag))
    np.testing.assert_allclose(fx[b], xk, rtol=1e-9, atol=1e-15, err_msg=str(tag))
    np.testing.assert_allclose(fP[b], P, rtol=1e-9, atol=1e-18, err_msg=str(tag))


def test_legacy_keep_feeds_the_zones_behind_the_grid(pkg, ofk, scene):
    """(d) of_module's loop: the rejects are the tracked points the legacy keep refused; the replacing detection runs through the grid
    with empty cells behind a mask of the zones alone."""
    from of_amd.of_library import pix_trans
    from of_amd.pipeline import PipelineConfig
    frames = scene[0]
    cfg = cc.of_module_cfg(PipelineConfig)
    inp = cc.of_module_inputs(pix_trans)
    fs, fusion = of_module_stream(ofk, frames, cfg, inp, NB)
    try:
        logs = [[] for _ in range(NB)]
        refs = [cc.of_module_reference(frames[b], cfg, inp, b, fusion.model, grid_log=logs[b]) for b in range(NB)]
        used = [1] * NB                                          # the next entry of the stream's grid log (0: the first detection)
        tracks, counts = fs.begin(frames[:, 0])
        st = fs.corner_grid_stats()
        for b in range(NB):
            assert counts[b] == len(refs[b][0]) and np.array_equal(bits(tracks[b, :counts[b]]), bits(refs[b][0])) and tuple(int(v) for v in st[b]) == tuple(logs[b][0])
        tot = dict(inserted=0, masked=0, rejects=0, bound=0)
        for t in range(1, cc.NF):
            rec, fused, tracks, counts = fs.step_fused(frames[:, t], of_module_sensors(ofk, inp, t, NB))
            zones, grid = fs.zones(), fs.corner_grid_stats()
            fx, fP = fs.ctx.filter_state(NB)
            for b in range(NB):
                s = refs[b][1][t - 1]; z = s[6]; tag = ("legacy", t, b)
                assert_of_module_step(rec, fused, tracks, counts, fx, fP, b, s, tag)
                assert_zones_equal(zones, b, z["zones"], tag)
                if z["redetected"]:
                    want = logs[b][used[b]]; used[b] += 1
                    assert tuple(int(v) for v in grid[b]) == tuple(want), (tag, grid[b], want)
                    tot["bound"] += int(want[1] > want[0])
                tot["inserted"] += int(z["zones"].stats[1]); tot["rejects"] += z["rejects"]; tot["masked"] += int(z["redetected"] and z["zones_masked"] > 0)
        print(f"legacy keep: zones inserted {tot['inserted']}, rejects {tot['rejects']}, replacing detections behind a zone mask {tot['masked']}, grid bound in {tot['bound']}")
        assert min(tot.values()) > 0 and fs.ctx.get_robust().loss == ofk.ROBUST_OFF
    finally:
        fs.close()


def test_held_step_leaves_the_zone_table_untouched(pkg, ofk, scene):
    """(e) one stream with hold_on_skip: the step whose control throws the predicted velocity off finds nothing feasible and is held;
    behind it zones() returns the bits it returned before it, the age (ttl, offset) included; the steps that follow equal the
    reference with its table.  (A reference that aged the table on the held step differs: test_combined_reference.py.)"""
    from of_amd.of_library import pix_trans
    from of_amd.pipeline import PipelineConfig
    frames = scene[0][1:2]
    cfg = cc.of_module_cfg(PipelineConfig, grid=None)
    inp = cc.of_module_inputs(pix_trans, nb=1, held=True)
    fs, fusion = of_module_stream(ofk, frames, cfg, inp, 1, hold=True)
    try:
        first, steps = cc.of_module_reference(frames[0], cfg, inp, 0, fusion.model, hold=True)
        tracks, counts = fs.begin(frames[:, 0])
        assert counts[0] == len(first) and np.array_equal(bits(tracks[0, :counts[0]]), bits(first))
        before, held, inserted_after = None, 0, 0
        for t in range(1, cc.NF):
            rec, fused, tracks, counts = fs.step_fused(frames[:, t], of_module_sensors(ofk, inp, t, 1))
            zones = fs.zones()
            fx, fP = fs.ctx.filter_state(1)
            s = steps[t - 1]; tag = ("held", t)
            assert_of_module_step(rec, fused, tracks, counts, fx, fP, 0, s, tag)
            assert_zones_equal(zones, 0, s[6]["zones"], tag)
            if s[6]["held"]:
                held += 1
                assert t == cc.HELD_STEP and rec[0, 15] == 0 and np.count_nonzero(before["zones"][0, :, 0]) > 0, tag
                for k in ("zones", "motion", "stats"):
                    assert np.array_equal(bits(zones[k]), bits(before[k])), (tag, k)
            elif held:
                inserted_after += int(zones["stats"][0, 1])
            before = zones
        print(f"held step {cc.HELD_STEP}: live zones across it {int(np.count_nonzero(steps[cc.HELD_STEP - 1][6]['zones'].zones[:, 0]))}, zones inserted behind it {inserted_after}")
        assert held == 1 and inserted_after > 0
    finally:
        fs.close()


def test_begin_clears_the_zone_table(pkg, ofk, scene):
    """(f) a second ofk_stream_begin on a stream that holds live zones reads an all-zero table, and the steps behind it are a fresh
    stream's bit for bit."""
    from of_amd.pipeline import FlowStream, PipelineConfig
    frames, info, sr = scene
    cfg = PipelineConfig(**cc.CASES["grid-zones"]["cfg"])
    fs = FlowStream(W, H, batch=NB, cfg=cfg, min_features=cc.MIN_FEAT, mask_radius=cc.RADIUS)
    try:
        runs = []
        for again in (False, True):
            out = [fs.begin(frames[:, 0])]
            z = fs.zones()
            assert not z["zones"].any() and not z["motion"].any() and not z["stats"].any(), again
            for t in range(1, 4):
                out.append(fs.step(frames[:, t], sr) + (fs.zones(),))
            runs.append(out)
            live = int(np.count_nonzero(out[-1][3]["zones"][:, :, 0]))
            assert live > 0                                      # the run leaves live zones behind
        print(f"begin: live zones cleared {live}")
        def same_tracks(t0, c0, t1, c1):                         # rows past a stream's count are not part of the answer (ofk.h)
            return np.array_equal(c0, c1) and all(np.array_equal(bits(t0[b, :c0[b]]), bits(t1[b, :c0[b]])) for b in range(NB))
        assert same_tracks(*runs[0][0], *runs[1][0])
        for (r0, t0, c0, z0), (r1, t1, c1, z1) in zip(runs[0][1:], runs[1][1:]):
            assert same_tracks(t0, c0, t1, c1) and np.array_equal(bits(r0), bits(r1))
            assert all(np.array_equal(bits(z0[k]), bits(z1[k])) for k in ("zones", "motion", "stats"))
    finally:
        fs.close()


def pair_setup(ofk, gpu_ctx, scene):
    if "pairs" not in _cache:
        from of_amd.pipeline import PipelineConfig
        frames, info, _ = scene
        B = len(cc.PAIR_FRAMES)
        sr = cc.sensor_rows(ofk, info, B)
        cfg = PipelineConfig(**cc.PAIR_CFG)
        prev, nxt = cc.pair_frames(frames)
        _cache["pairs"] = (cfg, prev, nxt, sr, cc.pair_references(cfg, prev, nxt, sr, predict=device_predict(gpu_ctx)), {})
    return _cache["pairs"]


@pytest.mark.parametrize("slices", [1, 2])
def test_frame_pairs_with_five_settings(pkg, ofk, gpu_ctx, scene, slices):
    """(g) seed + gate + grid + robust + cov through ofk_pairs_run: three pairs, so that two slices hold 1 and 2 of them and
    solve_pairs carves its per-slice offsets into the robust, covariance and gate buffers at a pair that is not the first."""
    from batch_oracle import assert_pair_matches
    from of_amd.pipeline import FlowPipeline
    cfg, prev, nxt, sr, refs, outs = pair_setup(ofk, gpu_ctx, scene)
    B = len(prev)
    pipe = FlowPipeline(W, H, B, cfg, streams=slices)
    try:
        pipe.upload(prev, nxt, sr)
        out = pipe.run()
        gstats, grid, cov = pipe.track_gate_stats(), pipe.corner_grid_stats(), pipe.covariances()
        wts, rst = pipe.ctx.robust_download(B)
        cfgd = cc.cov_dict(cfg)
        refused = zero = 0
        for b, r in enumerate(refs):
            tag = f"five settings, slices {slices}"
            assert_pair_matches(out, b, r, tag)
            n = len(r["pts"])
            assert np.array_equal(gstats[b], r["gate"]["stats"]) and tuple(int(v) for v in grid[b]) == tuple(r["grid_stats"]), (tag, b, gstats[b], grid[b])
            np.testing.assert_array_equal(rst[b, [3, 4, 6, 7]], r["robust"]["stats"][[3, 4, 6, 7]], err_msg=tag)
            np.testing.assert_allclose(wts[b, :n], r["weights"], rtol=0, atol=1e-9, err_msg=tag)
            assert not wts[b, n:].any()
            want = cr.pair_record(cr.NODE, out["prev_pts"][b, :n], out["next_pts"][b, :n], out["status"][b, :n], sr[b], cfgd, out["records"][b], w=wts[b, :n])
            assert want[13] == 0 and cr.condition(cr.NODE, out["prev_pts"][b, :n], out["next_pts"][b, :n], (out["status"][b, :n] == 1) & (wts[b, :n] > 0), sr[b], w=wts[b, :n]) < 1e3
            assert_cov_close(cov[b], want, f"{tag} pair {b}")
            refused += int(np.count_nonzero((r["gate"]["st_f"] == 1) & (r["status"] == 0))); zero += int(np.count_nonzero((r["status"] == 1) & (r["weights"] == 0)))
        print(f"pairs, slices {slices}: gate-refused {refused}, tracked points of weight 0 {zero}, grid examined/accepted "
              f"{[tuple(int(v) for v in g[::-1]) for g in grid]}")
        assert refused > 0 and zero > 0
        # ofk_pairs_run ignores the zones setting: no output bit changes, and the table a later download reads was never written
        pipe.ctx.set_zones(mode="hull")
        again = pipe.run()
        for k in ("records", "prev_pts", "next_pts", "status", "err", "counts"):
            assert np.array_equal(bits(again[k]), bits(out[k])), k
        assert np.array_equal(bits(pipe.covariances()), bits(cov)) and np.array_equal(bits(pipe.ctx.robust_download(B)[0]), bits(wts))
        z = pipe.ctx.zones_download(B)
        assert not z["zones"].any() and not z["motion"].any() and not z["stats"].any()
        outs[slices] = (out, cov, wts)
        if len(outs) == 2:                                       # both launch forms: the same bits
            (o1, c1, w1), (o2, c2, w2) = outs[1], outs[2]
            for k in ("records", "prev_pts", "next_pts", "status", "err", "counts"):
                assert np.array_equal(bits(o1[k]), bits(o2[k])), k
            assert np.array_equal(bits(c1), bits(c2)) and np.array_equal(bits(w1), bits(w2))
    finally:
        pipe.close()


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
def test_all_six_set_and_switched_off_equals_never_set(pkg, ofk, scene, fused):
    """(h) the six per-feature "off means off" tests in one: every setting on, then every setting off, before begin."""
    from of_amd.pipeline import FlowStream, PipelineConfig, FusionConfig
    frames, info, sr = scene
    plain = PipelineConfig(**cc.BASE)
    allon = PipelineConfig(**cc.CASES["all-step"]["cfg"])
    res = []
    for touch in (False, True):
        fs = FlowStream(W, H, batch=NB, cfg=plain, min_features=cc.MIN_FEAT, mask_radius=cc.RADIUS, fusion=FusionConfig(use_imu=False) if fused else None)
        try:
            c = fs.ctx
            if touch:
                c.set_lk_seed(allon.lk_seed, allon.seed_gain); c.set_robust(allon.robust_setting()); c.set_track_gate(allon.track_gate_setting())
                c.set_corner_grid(allon.corner_grid_setting()); c.set_cov(allon.cov_setting()); c.set_zones(allon.zones_setting())
                c.set_lk_seed("off"); c.set_robust(None); c.set_track_gate(None); c.set_corner_grid(None); c.set_cov(None); c.set_zones(None)
                assert c.get_lk_seed()[0] == ofk.SEED_OFF and c.get_robust().loss == ofk.ROBUST_OFF and c.get_track_gate().fb_mode == ofk.FB_OFF
                assert c.get_corner_grid().cell == 0 and c.get_cov().mode == ofk.COV_OFF and c.get_zones().mode == ofk.ZONES_OFF
            steps = [fs.begin(frames[:, 0])]
            for t in range(1, 4):
                steps.append(fs.step_fused(frames[:, t], sr) if fused else fs.step(frames[:, t], sr))
            res.append(steps)
        finally:
            fs.close()
    for a, b in zip(*res):
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))
