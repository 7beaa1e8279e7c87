"""GPU: the velocity covariance (ofk_set_cov / ofk_velocity_solve_cov) against tests/cov_reference.py.

Every entry of a device covariance lies within 1e-9 of the matrix's largest entry: the f64 sums of at most 4096 terms carry about
2e-16 n cond(M) of rounding, the scenes have cond(M) < 1e3 (asserted here on the CPU side), so rounding stays below 1e-10 while a wrong
term is off by orders of magnitude more.  The resident paths feed the reference with the points, status and sensors the device
downloaded; their image stages have their own suites."""
import numpy as np
import pytest

import cov_reference as cr
from oracle import estimation_oracle as eo
from point_stage_helpers import bits

pytestmark = pytest.mark.gpu

TOL = 1e-9
COND_MAX = 1e3
SIG = dict(sigma_flow=0.002, sigma_pos=0.003, sigma_d=0.04, sigma_omega=(0.01, 0.02, 0.015), sigma_normal=0.004, sigma_offset=0.006)
SIG_PX = dict(SIG, sigma_flow=0.3, sigma_pos=0.5)                # the resident paths take pixels
SEEN = dict(dev=0.0)


def assert_cov_close(got, ref, tag):
    """Slots 0-5, 6-11 and 16-21 each within TOL of their block's largest entry; s^2 relative; flags equal."""
    assert got[13] == ref[13], (tag, "flag", got[13], ref[13])
    assert got[22] == 0 and got[23] == 0, tag
    for sl in (slice(0, 6), slice(6, 12), slice(16, 22)):
        scale = np.abs(ref[sl]).max()
        dev = np.abs(got[sl] - ref[sl]).max() / scale if scale > 0 else np.abs(got[sl]).max()
        SEEN["dev"] = max(SEEN["dev"], dev)
        assert dev <= TOL, (tag, sl, dev, got[sl], ref[sl])
    assert abs(got[12] - ref[12]) <= TOL * abs(ref[12]), (tag, "s2", got[12], ref[12])


def scene(n, seed, variant):
    """n points spread over the image plane (the first four on the corners of a square, so that small n are well conditioned)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.7, 0.7, (n, 2))
    x[:min(n, 4)] = np.array([[0.8, 0.8], [-0.8, -0.8], [0.8, -0.8], [-0.8, 0.8]])[:min(n, 4)]
    nrm = np.array([0.05, -0.08, 1.0]) + rng.normal(0, 0.02, 3); nrm /= np.linalg.norm(nrm)
    om = rng.normal(0, 0.15, 3); v = rng.normal(0, 0.4, 3); d = float(rng.uniform(0.8, 3.0)); t = rng.normal(0, 0.1, 3)
    u = eo.generate_test_data(x, v, om, d, nrm) + rng.normal(0, 1e-3, (n, 2))
    return x, u, d, nrm, om, t


def batch3(n, variant):
    sc = [scene(n, 100 * n + b, variant) for b in range(3)]
    return tuple(np.stack([s[k] for s in sc]) for k in range(6))


NS = (2, 3, 8, 63, 64, 65, 257, 500, 4096)


@pytest.mark.parametrize("n", NS)
def test_stage_entry(gpu_ctx, ofk, n):
    for variant in (ofk.SOLVE_NODE, ofk.SOLVE_SIM):
        x, u, d, nrm, om, t = batch3(n, variant)
        mask = np.ones((3, n), np.uint8); mask[:, 2::3] = 0         # every third point from the third on is skipped
        for valid in (None, mask):
            for lever in (None, t):
                for mode in (ofk.COV_PROPAGATE, ofk.COV_RESIDUAL):
                    out, cov = gpu_ctx.velocity_solve_cov(variant, x, u, d=d, nrm=nrm, omega=om, t=lever, valid=valid, mode=mode, **SIG)
                    plain = gpu_ctx.velocity_solve(variant, x, u, d=d, nrm=nrm, omega=om, t=lever, valid=valid)
                    assert np.array_equal(bits(out), bits(plain))
                    for b in range(3):
                        tag = f"n {n} variant {variant} valid {valid is not None} lever {lever is not None} mode {mode} problem {b}"
                        keep = np.ones(n, bool) if valid is None else valid[b].astype(bool)
                        M, _ = cr.normal_equations(variant, x[b][keep], u[b][keep], d[b], nrm[b], om[b])
                        assert np.linalg.cond(M) < COND_MAX, tag
                        v = out[b, :3] + (np.cross(om[b], lever[b]) if lever is not None else 0.0)
                        ref = cr.covariance(variant, x[b], u[b], d[b], nrm[b], om[b], cr.sigmas(**SIG), mode, v=v, rss=out[b, 3], rank=out[b, 4],
                                            t=None if lever is None else lever[b], valid=None if valid is None else valid[b])
                        if mode == ofk.COV_RESIDUAL and 2 * keep.sum() <= 3:
                            assert np.array_equal(cov[b], cr.void_record()), tag
                        else:
                            assert ref[13] == 0, tag
                            assert_cov_close(cov[b], ref, tag)
    print(f"n {n}: largest deviation so far {SEEN['dev']:.3e} of a block's largest entry")


def test_stage_entry_with_the_robust_setting(gpu_ctx, ofk):
    n = 500
    x, u, d, nrm, om, t = batch3(n, ofk.SOLVE_NODE)
    rng = np.random.default_rng(9)
    u[:, 5::9] += rng.normal(0, 0.05, u[:, 5::9].shape)           # outliers for the reweighting to reject
    setting = ofk.robust_setting("tukey", hypotheses=32, seed=77)
    out_r, w, st = gpu_ctx.velocity_solve_robust(ofk.SOLVE_NODE, x, u, d=d, nrm=nrm, omega=om, t=t, robust=setting)
    out, cov = gpu_ctx.velocity_solve_cov(ofk.SOLVE_NODE, x, u, d=d, nrm=nrm, omega=om, t=t, robust=setting, mode="propagate", **SIG)
    assert np.array_equal(bits(out), bits(out_r)) and np.any(w == 0) and np.any((w > 0) & (w < 1))
    for mode in (ofk.COV_PROPAGATE, ofk.COV_RESIDUAL):
        out, cov = gpu_ctx.velocity_solve_cov(ofk.SOLVE_NODE, x, u, d=d, nrm=nrm, omega=om, t=t, robust=setting, mode=mode, **SIG)
        for b in range(3):
            M, _ = cr.normal_equations(cr.NODE, x[b], u[b], d[b], nrm[b], om[b], w[b])
            assert np.linalg.cond(M) < COND_MAX
            ref = cr.covariance(cr.NODE, x[b], u[b], d[b], nrm[b], om[b], cr.sigmas(**SIG), mode, v=out[b, :3] + np.cross(om[b], t[b]),
                                rss=out[b, 3], rank=out[b, 4], t=t[b], w=w[b])
            assert_cov_close(cov[b], ref, f"robust mode {mode} problem {b}")


def test_stage_entry_void_and_refused(gpu_ctx, ofk):
    x, u, d, nrm, om, t = batch3(8, ofk.SOLVE_NODE)
    # one point: rank 2
    out, cov = gpu_ctx.velocity_solve_cov(ofk.SOLVE_NODE, x[:, :1], u[:, :1], d=d, nrm=nrm, omega=om, mode="propagate", **SIG)
    assert np.array_equal(bits(out), bits(gpu_ctx.velocity_solve(ofk.SOLVE_NODE, x[:, :1], u[:, :1], d=d, nrm=nrm, omega=om)))
    assert np.all(out[:, 4] < 3) and all(np.array_equal(c, cr.void_record()) for c in cov)
    # one problem without a valid point beside two ordinary ones
    valid = np.ones((3, 8), np.uint8); valid[1] = 0
    out, cov = gpu_ctx.velocity_solve_cov(ofk.SOLVE_SIM, x, u, d=d, nrm=nrm, omega=om, t=t, valid=valid, mode="residual", **SIG)
    assert np.array_equal(bits(out), bits(gpu_ctx.velocity_solve(ofk.SOLVE_SIM, x, u, d=d, nrm=nrm, omega=om, t=t, valid=valid)))
    assert np.array_equal(cov[1], cr.void_record()) and cov[0, 13] == 0 and cov[2, 13] == 0 and out[1, 4] == 0
    # d = 0 is void
    out, cov = gpu_ctx.velocity_solve_cov(ofk.SOLVE_NODE, x, u, d=np.array([1.0, 0.0, 2.0]), nrm=nrm, omega=om, mode="propagate", **SIG)
    assert np.array_equal(cov[1], cr.void_record()) and cov[0, 13] == 0
    for bad in (dict(variant=ofk.SOLVE_OFMODULE), dict(mode=7), dict(mode="off"), dict(sigma_d=-1.0), dict(sigma_flow=np.nan), dict(filter_r=True),
                dict(nis_max=np.inf)):
        kw = dict(SIG, mode="propagate"); kw.update({k: v for k, v in bad.items() if k != "variant"})
        with pytest.raises((ofk.OfkError, ValueError)):
            gpu_ctx.velocity_solve_cov(bad.get("variant", ofk.SOLVE_NODE), x, u, d=d, nrm=nrm, omega=om, **kw)


# ---------------------------------------------------------------------------------------------------- resident pairs
H, W, CORNERS = 120, 160, 64
MOTION = dict(v=(0.004, -0.003, 0.002), omega=(0.003, -0.002, 0.004), d=1.0)
_frames = {}


def pair_frames(B):
    if "pairs" not in _frames:
        from of_amd import synth
        _frames["pairs"] = synth.make_batch(130, H, W, seed=7300, distinct=4, margin=48, **MOTION)
    prev, nxt, base = _frames["pairs"]
    return prev[:B], nxt[:B], base


def pair_sensors(ofk, B, base):
    p0 = base[0]
    R = eo.quat_to_rot(0.1, -0.05, 0.2, np.sqrt(1 - 0.01 - 0.0025 - 0.04))
    return ofk.make_sensors(B, d=p0["d"], normal=p0["n"], omega=p0["omega"], rotation=R, offset=(0.02, -0.01, 0.2), scaling=p0["scaling"],
                            cx=p0["cx"], cy=p0["cy"], v_prior=p0["v"])


def run_pairs(ofk, B, cov, slices=1, feas=False, robust=None, gate=None):
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    prev, nxt, base = pair_frames(B)
    cfg = PipelineConfig(max_corners=CORNERS, quality=0.01, min_distance=6, block_size=5, win=15, max_level=2, max_count=20, eps=0.03,
                         use_feasibility=feas, feas_T=-0.8)
    sensors = pair_sensors(ofk, B, base)
    pipe = FlowPipeline(W, H, B, cfg, streams=slices)
    try:
        if robust:
            pipe.ctx.set_robust(**robust)
        if gate:
            pipe.ctx.set_track_gate(**gate)
        pipe.upload(prev, nxt, sensors)
        plain = pipe.run()
        with pytest.raises(ofk.OfkError):
            pipe.covariances()                                   # nothing ran with the setting on yet
        pipe.ctx.set_cov(**cov)
        out = pipe.run()
        rec = pipe.covariances()
        wts = pipe.ctx.robust_download(B)[0] if robust else None
        pipe.ctx.set_cov(None)
        again = pipe.run()
    finally:
        pipe.close()
    for k in ("records", "prev_pts", "next_pts", "status", "err", "counts"):     # fields 0-15 and the image outputs: the setting changes none
        assert np.array_equal(bits(out[k]), bits(plain[k])), k
        assert np.array_equal(bits(again[k]), bits(plain[k])), k
    return sensors, out, rec, wts


PAIR_CASES = [
    pytest.param(dict(mode="propagate"), {}, id="propagate"),
    pytest.param(dict(mode="residual"), dict(slices=2), id="residual-2slices"),
    pytest.param(dict(mode="propagate"), dict(feas=True), id="feasibility"),
    pytest.param(dict(mode="propagate"), dict(robust=dict(loss="huber", hypotheses=16, seed=5), gate=dict(fb="plain", fb_thr=0.5)), id="robust-gate"),
]


@pytest.mark.parametrize("cov,kw", PAIR_CASES)
def test_resident_pairs(pkg, ofk, cov, kw):
    setting = dict(SIG_PX, **cov)
    cfgd = dict(setting, mode=ofk.COV_MODES[cov["mode"]])
    got = {}
    for B in (3, 130):                                           # the workgroup form and the one-wave form
        sensors, out, rec, wts = run_pairs(ofk, B, setting, **kw)
        got[B] = rec
        solved = 0
        for b in range(B if B == 3 else 12):                     # the reference on a dozen pairs; the rest by the bits below
            n = int(out["counts"][b])
            w = None if wts is None else wts[b, :n]
            ref = cr.pair_record(cr.NODE, out["prev_pts"][b, :n], out["next_pts"][b, :n], out["status"][b, :n], sensors[b], cfgd, out["records"][b],
                                 w=w, use_feas=kw.get("feas", False), feas_T=-0.8)
            if not kw.get("feas"):
                assert ref[13] == 0, (B, b)
            keep = out["status"][b, :n] == 1
            if w is not None:
                keep = keep & (w > 0)
            if not kw.get("feas"):
                assert cr.condition(cr.NODE, out["prev_pts"][b, :n], out["next_pts"][b, :n], keep, sensors[b], w=w) < COND_MAX
            assert_cov_close(rec[b], ref, f"{kw} B {B} pair {b}")
            solved += int(ref[13] == 0)
        assert solved and out["records"][0, 11] >= 8
        if kw.get("feas"):
            assert np.any(out["records"][:, 11] < out["records"][:, 13])      # the feasibility test dropped points
    assert np.array_equal(bits(got[3]), bits(got[130][:3]))      # the same pair in both launch forms: the same bits
    # pairs 4.. are cyclic shifts of the first four: all solved
    assert kw.get("feas") or np.all(got[130][:, 13] == 0)
    print(f"{kw}: largest deviation so far {SEEN['dev']:.3e}")


def test_pairs_filter_step(pkg, ofk):
    from of_amd.pipeline import FlowPipeline, PipelineConfig, FilterModel
    B = 3
    prev, nxt, base = pair_frames(B)
    cfg = PipelineConfig(max_corners=CORNERS, quality=0.01, min_distance=6, block_size=5, win=15, max_level=2, max_count=20, eps=0.03)
    sensors = pair_sensors(ofk, B, base)
    model = FilterModel.kf3()
    model.R = 1e-4 * np.eye(3); model.P0 = 1e-4 * np.eye(3)
    results = {}
    for name, cov in (("const", None), ("plain_r", dict(SIG_PX, mode="propagate")), ("filter_r", dict(SIG_PX, mode="propagate", filter_r=True, r_floor=1e-7)),
                      ("gate_all", dict(SIG_PX, mode="propagate", filter_r=True, nis_max=1e-300)),
                      ("gate_none", dict(SIG_PX, mode="propagate", filter_r=True, r_floor=1e-7, nis_max=1e300))):
        pipe = FlowPipeline(W, H, B, cfg)
        try:
            pipe.ctx.filter_configure(model, B)
            if cov:
                pipe.ctx.set_cov(**cov)
            pipe.upload(prev, nxt, sensors)
            out = pipe.run()
            pipe.ctx.pairs_filter_step(B, z_sign=-1.0, z_source=1)
            x, P = pipe.ctx.filter_state(B)
            results[name] = (out, x, P, pipe.covariances() if cov else None)
        finally:
            pipe.close()
    out, x_c, P_c, _ = results["const"]
    assert np.array_equal(bits(results["plain_r"][1]), bits(x_c)) and np.array_equal(bits(results["plain_r"][2]), bits(P_c))     # R_eff = R: the same bits
    assert np.array_equal(bits(results["gate_none"][1]), bits(results["filter_r"][1])) and np.array_equal(bits(results["gate_none"][3]), bits(results["filter_r"][3]))
    for name in ("plain_r", "filter_r", "gate_all"):
        _, x, P, rec = results[name]
        cov = dict(SIG_PX, mode=ofk.COV_PROPAGATE, filter_r=name != "plain_r", r_floor=1e-7 if name == "filter_r" else 0.0, nis_max=1e-300 if name == "gate_all" else 0.0)
        for b in range(B):
            xp, Pp = eo.kf_predict(np.array(model.x0), np.array(model.P0), model.F, model.Q)
            z = -out["records"][b, 8:11]
            xr, Pr, nis, gated = cr.kf_correct_cov(xp, Pp, model.H, model.R, z, cov_rec=rec[b], z_sign=-1.0, z_source=1, filter_r=cov["filter_r"],
                                                   r_floor=cov["r_floor"], nis_max=cov["nis_max"])
            np.testing.assert_allclose(x[b], xr, rtol=1e-9, atol=1e-15); np.testing.assert_allclose(P[b], Pr, rtol=1e-9, atol=1e-18)
            assert rec[b, 15] == gated == (1.0 if name == "gate_all" else 0.0) and abs(rec[b, 14] - nis) <= 1e-9 * nis and nis > 0
            if name == "gate_all":
                assert np.array_equal(x[b], xp) and np.array_equal(P[b], Pp)
    assert not np.allclose(results["filter_r"][1], x_c, rtol=1e-6)        # the covariance moved the gain


# ---------------------------------------------------------------------------------------------------- the fused stream step
def stream_run(ofk, cov, gps=False, msgs_on=True, touch_only=False):
    """2 streams x 4 frames with FusionConfig.ekf6; returns per step what the device reported and what the reference loop needs."""
    from of_amd import synth
    from of_amd.pipeline import FlowStream, PipelineConfig, FusionConfig
    from stream_oracle import imu_messages
    B, T = 2, 4
    if "stream" not in _frames:
        seqs = [synth.render_sequence(H, W, 7400 + s, T, margin=64, **MOTION) for s in range(B)]
        _frames["stream"] = (np.stack([s[0] for s in seqs]), seqs[0][1])
    frames, info = _frames["stream"]
    cfg = PipelineConfig(max_corners=CORNERS, quality=0.01, min_distance=6, block_size=5, win=15, max_level=2, max_count=20, eps=0.03)
    fusion = FusionConfig.ekf6(gps=gps, r=1e-4, p0=1e-4)
    sensors = ofk.make_sensors(B, d=info["d"], normal=info["n"], omega=info["omega"], offset=(0.02, -0.01, 0.2), scaling=info["scaling"],
                               cx=info["cx"], cy=info["cy"], v_prior=(0.004, -0.003, 0.002))
    fs = FlowStream(W, H, batch=B, cfg=cfg, min_features=10, mask_radius=8, fusion=fusion)
    steps = []
    try:
        if cov is not None:
            fs.ctx.set_cov(**cov)
            if touch_only:
                fs.ctx.set_cov(None)
        tracks, counts = fs.begin(frames[:, 0])
        rng = np.random.default_rng(31)
        for t in range(1, T):
            msgs = np.stack([imu_messages(rng, 0.1 * t + 10 * s, 3, rate=info["omega"]) for s in range(B)])
            fs.push_imu(msgs)
            imu, dv = fs.ctx.imu_state(B)
            old_tracks, old_counts = tracks.copy(), counts.copy()
            rec, fused, tracks, counts = fs.step_fused(frames[:, t], sensors)
            nxt, keep = fs.ctx.stream_last_points(CORNERS)
            x, P = fs.ctx.filter_state(B)
            steps.append(dict(rec=rec, fused=fused, old=old_tracks, n=old_counts, nxt=nxt, keep=keep, imu=imu, dv=dv, x=x, P=P,
                              cov=fs.covariances() if cov is not None and not touch_only else None))
    finally:
        fs.close()
    return steps, sensors, fusion


STREAM_CASES = [
    pytest.param(dict(filter_r=True, r_floor=1e-8), True, id="filter_r-gps"),
    pytest.param(dict(filter_r=True, omega_from_imu=True), False, id="omega-from-imu"),
    pytest.param(dict(filter_r=False), False, id="nis-only"),
    pytest.param(dict(filter_r=True, nis_max=1e-300), False, id="gate-all"),
]


@pytest.mark.parametrize("extra,gps", STREAM_CASES)
def test_fused_stream_step(pkg, ofk, extra, gps):
    setting = dict(SIG_PX, mode="propagate", **extra)
    steps, sensors, fusion = stream_run(ofk, setting, gps=gps)
    cfgd = dict(setting, mode=ofk.COV_PROPAGATE)
    solved = 0
    for s in range(2):
        loop = cr.CovStreamLoop(fusion.model, cfgd, fusion.z_sign, fusion.z_source)
        for k, st in enumerate(steps):
            n = int(st["n"][s])
            tag = f"{extra} stream {s} step {k}"
            xp, Pp = eo.kf_predict(loop.x, loop.P, fusion.model.F, fusion.model.Q, fusion.model.B, st["dv"][s])
            cv, x, P, fused = loop.step(st["old"][s, :n], st["nxt"][s, :n], st["keep"][s, :n], sensors[s], st["rec"][s], st["dv"][s], imu=st["imu"][s])
            assert st["rec"][s, 15] == 1 and cv[13] == 0, tag
            keep = st["keep"][s, :n].astype(bool)
            assert cr.condition(cr.NODE, st["old"][s, :n], st["nxt"][s, :n], keep, sensors[s], nrm=st["imu"][s, 15:18], omega=st["imu"][s, 18:21]) < COND_MAX
            assert_cov_close(st["cov"][s], cv, tag)
            assert st["cov"][s, 15] == cv[15] and abs(st["cov"][s, 14] - cv[14]) <= 1e-9 * cv[14] and cv[14] > 0, (tag, st["cov"][s, 14:16], cv[14:16])
            np.testing.assert_allclose(st["x"][s], x, rtol=1e-9, atol=1e-15, err_msg=tag)
            np.testing.assert_allclose(st["P"][s], P, rtol=1e-9, atol=1e-18, err_msg=tag)
            np.testing.assert_allclose(st["fused"][s], fused, rtol=1e-9, atol=1e-15, err_msg=tag)
            if extra.get("nis_max"):
                assert cv[15] == 1 and np.allclose(st["x"][s], xp, rtol=1e-9, atol=0) and np.allclose(st["P"][s], Pp, rtol=1e-9, atol=0), tag
            solved += 1
    assert solved == 6
    if extra.get("omega_from_imu"):                              # the pushed messages carry 1e-4, 2e-4, 3e-4: not the setting's sigmas
        assert np.allclose(steps[0]["imu"][:, 21:24], [1e-4, 2e-4, 3e-4])
        other, _, _ = stream_run(ofk, dict(setting, omega_from_imu=False))
        assert not np.allclose(other[0]["cov"][:, 18], steps[0]["cov"][:, 18], rtol=1e-3)


def test_fused_stream_constant_r_bits_and_the_open_gate(pkg, ofk):
    base, _, _ = stream_run(ofk, None)
    plain, _, _ = stream_run(ofk, dict(SIG_PX, mode="propagate"))                     # R_eff = R, corrected by the covariance kernel
    for a, b in zip(base, plain):
        for k in ("rec", "fused", "x", "P", "nxt", "keep"):
            assert np.array_equal(bits(a[k]), bits(b[k])), k
    r0, _, _ = stream_run(ofk, dict(SIG_PX, mode="residual", filter_r=True, r_floor=1e-8))
    r1, _, _ = stream_run(ofk, dict(SIG_PX, mode="residual", filter_r=True, r_floor=1e-8, nis_max=1e300))
    for a, b in zip(r0, r1):
        for k in ("rec", "fused", "x", "P", "cov"):
            assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert not np.array_equal(bits(r0[-1]["x"]), bits(base[-1]["x"]))


def test_off_is_off_and_refusals(pkg, ofk):
    from of_amd.pipeline import FlowStream, PipelineConfig, FusionConfig
    base, _, _ = stream_run(ofk, None)
    touched, _, _ = stream_run(ofk, dict(SIG_PX, mode="propagate", filter_r=True), touch_only=True)
    for a, b in zip(base, touched):
        for k in ("rec", "fused", "x", "P", "nxt", "keep"):
            assert np.array_equal(bits(a[k]), bits(b[k])), k
    c = ofk.Context(0, W, H, 2, CORNERS, 2)
    try:
        assert c.get_cov().mode == ofk.COV_OFF
        with pytest.raises(ofk.OfkError):
            c.cov_download(2)
        c.set_cov(mode="residual", sigma_d=0.5, sigma_omega=(1, 2, 3), nis_max=4.0)
        for bad in (dict(mode=5), dict(mode="propagate", sigma_pos=-1e-9), dict(mode="propagate", r_floor=np.inf), dict(mode="off", filter_r=True),
                    dict(mode="propagate", nis_max=np.nan)):
            with pytest.raises(ofk.OfkError):
                c.set_cov(**bad)
            g = c.get_cov()
            assert (g.mode, g.sigma_d, list(g.sigma_omega), g.nis_max, g.filter_r) == (ofk.COV_RESIDUAL, 0.5, [1.0, 2.0, 3.0], 4.0, 0)
        raw = ofk.cov_setting("propagate")
        for field, val in (("omega_from_imu", 2), ("filter_r", -1)):
            setattr(raw, field, val)
            with pytest.raises(ofk.OfkError):
                c.set_cov(raw)
            setattr(raw, field, 0)
        c.set_cov(None)
        assert c.get_cov().mode == ofk.COV_OFF
    finally:
        c.close()
    # the of_module loop is not the sensor model: refused with a setting on
    fs = FlowStream(W, H, batch=1, cfg=PipelineConfig.of_module(), fusion=FusionConfig.of_module())
    try:
        fs.ctx.set_cov(mode="propagate")
        prev, nxt, _ = pair_frames(1)
        fs.begin(prev)
        with pytest.raises(ofk.OfkError, match="sensor model"):
            fs.step_fused(nxt, ofk.make_sensors(1))
    finally:
        fs.close()
