"""GPU: the joint velocity and rotation solve (ofk_set_joint / ofk_velocity_solve_joint) against tests/joint_reference.py.

(v, omega^) of the device lie within TOL of the restatement's, in the measure of joint_reference.rel_dev: TOL is the tolerance
tests/test_joint_reference.py pins on the CPU (16 x the largest deviation of the restatement from a stacked lstsq).  The residual sum
of squares is held to RSS_TOL = 1e-10 relative: it is stationary in (v, omega^) at the minimum, so only the rounding of a sum of at
most 1025 f64 terms (n eps = 2.3e-13) and the square of TOL reach it - plus an absolute floor for fits that are exact (3 points, or
no noise), where the sum is rounding alone: every one of the 3 m residual components is a difference of terms of size `scale`
(the largest |b X q0|), off by at most (TOL + 8 eps) scale, so the sum moves by at most 3 m ((TOL + 8 eps) scale)^2.  The record's eigenvalues and covariances are held to REC_TOL =
1e-9 of their block's largest entry, tests/test_gpu_cov.py's bound with its argument: rounding of about 2e-16 n cond stays below 1e-10
at the conditions asserted here (COND_MAX), a wrong term is off by orders of magnitude more.  The resident paths feed the reference with
the points, status and sensors the device downloaded; their image stages have their own suites."""
import numpy as np
import pytest

import joint_reference as jr
from joint_checks import JOINT, SEEN, assert_joint_close
from oracle import estimation_oracle as eo
from point_stage_helpers import bits
from test_joint_reference import TOL

pytestmark = pytest.mark.gpu


def batch3(n, **kw):
    sc = [jr.scene(n, 500 * n + b, **kw) for b in range(3)]
    return tuple(np.stack([s[k] for s in sc]) for k in range(7))


@pytest.mark.parametrize("n", jr.COUNTS)
def test_stage_entry(gpu_ctx, ofk, n):
    x, u, d, nrm, om0, v, om = batch3(n)
    t = np.array([[0.02, -0.01, 0.2]] * 3)
    mask = np.ones((3, n), np.uint8)
    if n > 8:
        mask[:, 4::3] = 0                                        # every third point from the fifth on is skipped
    for variant in (ofk.SOLVE_NODE, ofk.SOLVE_SIM):
        for name, prior in jr.PRIORS.items():
            for valid, lever in ((None, None), (mask, t)):
                plain = gpu_ctx.velocity_solve(variant, x, u, d=d, nrm=nrm, omega=om0, valid=valid)
                before = gpu_ctx.velocity_solve(variant, x, u, d=d, nrm=nrm, omega=om0, t=lever, valid=valid)      # what the joint kernel finds in `out`
                out, rec = gpu_ctx.velocity_solve_joint(variant, x, u, d=d, nrm=nrm, omega=om0, t=lever, valid=valid, sigma_flow=jr.SIGMA_FLOW,
                                                        sigma_omega=prior)
                assert np.array_equal(bits(out[:, 4:8]), bits(plain[:, 4:8]))
                for b in range(3):
                    tag = f"n {n} variant {variant} prior {name} valid {valid is not None} problem {b}"
                    ref = jr.joint_solve(variant, x[b], u[b], d[b], nrm[b], om0[b], jr.SIGMA_FLOW, prior, v_s=plain[b, :3], rss_s=plain[b, 3],
                                         rank=plain[b, 4], valid=None if valid is None else valid[b])
                    assert ref["flag"] == 0, tag
                    vdev = out[b, :3] + (np.cross(rec[b, 0:3], lever[b]) if lever is not None else 0.0)
                    ref["rec"][6:9] = before[b, :3]              # slots 6-8 hold out's fields as they were: v_s less omega0 x t
                    assert_joint_close(vdev, out[b, 3], rec[b], ref, tag)
    print(f"n {n}: largest deviation of (v, omega^) so far {SEEN['dev']:.3e} (TOL {TOL:.2e})")


def test_stage_entry_with_the_robust_setting(gpu_ctx, ofk):
    n = 257
    x, u, d, nrm, om0, v, om = batch3(n, outliers=True)
    setting = ofk.robust_setting("tukey", hypotheses=32, seed=77)
    for variant in (ofk.SOLVE_NODE, ofk.SOLVE_SIM):
        out_r, w, st = gpu_ctx.velocity_solve_robust(variant, x, u, d=d, nrm=nrm, omega=om0, robust=setting)
        assert np.any((w > 0) & (w < 1))
        out, rec = gpu_ctx.velocity_solve_joint(variant, x, u, d=d, nrm=nrm, omega=om0, robust=setting, sigma_flow=jr.SIGMA_FLOW, sigma_omega=1e-3)
        for b in range(3):
            ref = jr.joint_solve(variant, x[b], u[b], d[b], nrm[b], om0[b], jr.SIGMA_FLOW, (1e-3,) * 3, v_s=out_r[b, :3], rss_s=out_r[b, 3], rank=out_r[b, 4],
                                 w=w[b])
            assert ref["flag"] == 0 and rec[b, 11] == np.count_nonzero(w[b] > 0)
            assert_joint_close(out[b, :3], out[b, 3], rec[b], ref, f"robust variant {variant} problem {b}")


def test_stage_entry_flags_and_held_axes(gpu_ctx, ofk):
    x, u, d, nrm, om0, v, om = batch3(20, noise=0.0)
    kw = dict(nrm=nrm, omega=om0, sigma_flow=jr.SIGMA_FLOW)
    # flag 1: one point; d = 0; a NaN range among finite problems, which keep their bits
    plain = gpu_ctx.velocity_solve(ofk.SOLVE_NODE, x[:, :1], u[:, :1], d=d, nrm=nrm, omega=om0)
    out, rec = gpu_ctx.velocity_solve_joint(ofk.SOLVE_NODE, x[:, :1], u[:, :1], d=d, **kw)
    assert np.array_equal(bits(out), bits(plain)) and np.all(rec[:, 10] == 1) and np.array_equal(rec[:, 0:3], om0) and np.all(rec[:, 11] == 1)
    good, grec = gpu_ctx.velocity_solve_joint(ofk.SOLVE_NODE, x, u, d=d, **kw)
    assert np.all(grec[:, 10] == 0)
    for bad in (0.0, np.nan):
        dd = d.copy(); dd[1] = bad
        plain = gpu_ctx.velocity_solve(ofk.SOLVE_NODE, x, u, d=dd, nrm=nrm, omega=om0)
        out, rec = gpu_ctx.velocity_solve_joint(ofk.SOLVE_NODE, x, u, d=dd, **kw)
        assert rec[1, 10] == 1 and np.array_equal(bits(out[1]), bits(plain[1])) and np.all(rec[1, 3:6] == 0) and np.all(rec[1, 12:] == 0)
        for b in (0, 2):
            assert np.array_equal(bits(out[b]), bits(good[b])) and np.array_equal(bits(rec[b]), bits(grec[b])), (bad, b)
    # exact flow: the truth comes back
    assert np.abs(good[:, :3] - v).max() <= 1e-12 and np.abs(grec[:, 0:3] - om).max() <= 1e-12
    # flag 2: collinear points, every axis free; a prior makes it a problem again
    s = np.linspace(-0.5, 0.5, 20)
    xl = np.broadcast_to(np.stack([s, 0.3 * s + 0.1], 1), (3, 20, 2)).copy()
    ul = np.stack([eo.generate_test_data(xl[b], v[b], om[b], d[b], nrm[b]) for b in range(3)])
    plain = gpu_ctx.velocity_solve(ofk.SOLVE_NODE, xl, ul, d=d, nrm=nrm, omega=om0)
    out, rec = gpu_ctx.velocity_solve_joint(ofk.SOLVE_NODE, xl, ul, d=d, **kw)
    assert np.all(plain[:, 4] == 3) and np.all(rec[:, 10] == 2) and np.array_equal(bits(out), bits(plain)) and np.array_equal(rec[:, 0:3], om0)
    assert np.all(rec[:, 12] > 0) and np.all(rec[:, 14] < np.sqrt(jr.EPS * 60) * rec[:, 12]) and np.all(rec[:, 15:27] == 0)
    assert np.all(gpu_ctx.velocity_solve_joint(ofk.SOLVE_NODE, xl, ul, d=d, sigma_omega=1e-3, **kw)[1][:, 10] == 0)
    # two points: rank 3 for v, a singular S with every axis free (flag 2); a prior makes it a problem again - against the reference
    x8, u8, d8, nrm8, om8, _, _ = (np.stack([jr.scene(8, 6 + b)[k] for b in range(3)]) for k in range(7))
    plain = gpu_ctx.velocity_solve(ofk.SOLVE_NODE, x8[:, :2], u8[:, :2], d=d8, nrm=nrm8, omega=om8)
    assert np.all(plain[:, 4] == 3)
    for name, want in (("free", 2), ("prior", 0)):
        out, rec = gpu_ctx.velocity_solve_joint(ofk.SOLVE_NODE, x8[:, :2], u8[:, :2], d=d8, nrm=nrm8, omega=om8, sigma_flow=jr.SIGMA_FLOW,
                                                sigma_omega=jr.PRIORS[name])
        for b in range(3):
            ref = jr.joint_solve(jr.NODE, x8[b, :2], u8[b, :2], d8[b], nrm8[b], om8[b], jr.SIGMA_FLOW, jr.PRIORS[name], v_s=plain[b, :3], rss_s=plain[b, 3],
                                 rank=plain[b, 4])
            assert ref["flag"] == want and rec[b, 11] == 2, (name, b, ref["flag"])
            if want == 2:                                        # the eigenvalues that are rounding alone are held to the size of the largest
                assert np.array_equal(bits(out[b]), bits(plain[b])) and abs(rec[b, 12] - ref["rec"][12]) <= 1e-9 * ref["rec"][12], (b, rec[b, 12:15])
                assert np.all(np.abs(rec[b, 13:15]) <= 1e-13 * rec[b, 12]), (b, rec[b, 12:15])
            assert_joint_close(out[b, :3], out[b, 3], rec[b], ref, f"two points {name} problem {b}")
    # a prior term that overflows: flag 1, out has the plain solve's bits, the record is the reference's to the bit
    x, u, d, nrm, om0, v, om = batch3(65)
    for variant in (ofk.SOLVE_NODE, ofk.SOLVE_SIM):
        plain = gpu_ctx.velocity_solve(variant, x, u, d=d, nrm=nrm, omega=om0)
        for prior in ((1e-160,) * 3, (1e-160, np.inf, 0.0)):
            out, rec = gpu_ctx.velocity_solve_joint(variant, x, u, d=d, nrm=nrm, omega=om0, sigma_flow=jr.SIGMA_FLOW, sigma_omega=prior)
            assert np.array_equal(bits(out), bits(plain)), (variant, prior)
            for b in range(3):
                ref = jr.joint_solve(variant, x[b], u[b], d[b], nrm[b], om0[b], jr.SIGMA_FLOW, prior, v_s=plain[b, :3], rss_s=plain[b, 3], rank=plain[b, 4])
                assert ref["flag"] == 1 and np.array_equal(bits(rec[b]), bits(ref["rec"])), (variant, prior, b, rec[b])
                assert not rec[b, 3:6].any() and not rec[b, 12:].any() and rec[b, 11] == 65
    # all axes held: the plain solve's bits; one axis held: its delta is exactly 0
    x, u, d, nrm, om0, v, om = batch3(65)
    kw = dict(nrm=nrm, omega=om0, sigma_flow=jr.SIGMA_FLOW)
    plain = gpu_ctx.velocity_solve(ofk.SOLVE_SIM, x, u, d=d, nrm=nrm, omega=om0, t=om)
    out, rec = gpu_ctx.velocity_solve_joint(ofk.SOLVE_SIM, x, u, d=d, t=om, sigma_omega=0.0, **kw)
    assert np.array_equal(bits(out), bits(plain)) and np.all(rec[:, 10] == 0) and np.all(rec[:, 3:6] == 0) and np.array_equal(rec[:, 0:3], om0)
    assert np.all(rec[:, 12:21] == 0) and np.all(rec[:, [21, 24, 26]] > 0)
    out, rec = gpu_ctx.velocity_solve_joint(ofk.SOLVE_SIM, x, u, d=d, sigma_omega=(np.inf, 0.0, 1e-3), **kw)
    assert np.all(rec[:, 4] == 0) and np.all(rec[:, 14] == 0) and np.all(rec[:, 13] > 0) and np.all(rec[:, 3] != 0) and np.all(rec[:, [18, 16, 19]] == 0)


# ---------------------------------------------------------------------------------------------------- resident pairs
H, W, CORNERS = 120, 160, 64                                     # tests/test_gpu_cov.py's frame
MOTION = dict(v=(0.004, -0.003, 0.002), omega=(0.003, -0.002, 0.004), d=1.0)
GYRO_OFF = np.array([1e-3, -1e-3, 5e-4])
_frames = {}


def pair_frames(B):
    if "pairs" not in _frames:
        from of_amd import synth
        _frames["pairs"] = synth.make_batch(2, H, W, seed=7300, distinct=2, margin=48, **MOTION)
    prev, nxt, base = _frames["pairs"]
    idx = np.arange(B) % 2                                       # batch 2 and batch 130 hold the same pairs
    return prev[idx], nxt[idx], base


def pair_sensors(ofk, B, base):
    p0 = base[0]
    R = eo.quat_to_rot(0.1, -0.05, 0.2, np.sqrt(1 - 0.01 - 0.0025 - 0.04))
    return ofk.make_sensors(B, d=p0["d"], normal=p0["n"], omega=np.asarray(p0["omega"]) + GYRO_OFF, rotation=R, offset=(0.02, -0.01, 0.2),
                            scaling=p0["scaling"], cx=p0["cx"], cy=p0["cy"], v_prior=p0["v"])


def run_pairs(ofk, B, joint, slices=1, overlap=True, feas=False, robust=None, gate=None, seed=None, camera=None, rshutter=None, fresh=True):
    """A run with the setting off, one with it on, one with it off again.  Returns sensors, the run with it on, the joint records, the
    robust weights, the points the solve stage read and the run with the setting off."""
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    prev, nxt, base = pair_frames(B)
    cfg = PipelineConfig(max_corners=CORNERS, quality=0.01, min_distance=6, block_size=5, win=15, max_level=2, max_count=20, eps=0.03,
                         use_feasibility=feas, feas_T=-0.8)
    sensors = pair_sensors(ofk, B, base)
    pipe = FlowPipeline(W, H, B, cfg, streams=slices)
    try:
        pipe.ctx.set_overlap(overlap)
        if robust:
            pipe.ctx.set_robust(**robust)
        if gate:
            pipe.ctx.set_track_gate(**gate)
        if seed:
            pipe.ctx.set_lk_seed(seed)
        if camera:
            pipe.ctx.set_camera(**camera)
        if rshutter:
            pipe.ctx.set_rolling_shutter(**rshutter)
        pipe.upload(prev, nxt, sensors)
        plain = pipe.run()
        with pytest.raises(ofk.OfkError):
            pipe.rotations()                                     # nothing ran with the setting on yet
        pipe.ctx.set_joint(**joint)
        out = pipe.run()
        rec = pipe.rotations()
        wts = pipe.ctx.robust_download(B)[0] if robust else None
        pts = pipe.ctx.camera_download(B) if camera else pipe.ctx.rs_download(B) if rshutter else (out["prev_pts"], out["next_pts"])
        pipe.ctx.set_joint(None)
        again = pipe.run()
    finally:
        pipe.close()
    for k in ("prev_pts", "next_pts", "status", "err", "counts"):                  # the image side: the setting changes none
        assert np.array_equal(bits(out[k]), bits(plain[k])), k
    for k in ("records", "prev_pts", "next_pts", "status", "err", "counts"):       # switched off: the bits of a context that never had it
        assert np.array_equal(bits(again[k]), bits(plain[k])), k
    keep = [4, 5, 6, 7, 11, 12, 13, 14, 15]
    assert np.array_equal(bits(out["records"][:, keep]), bits(plain["records"][:, keep]))
    return sensors, out, rec, wts, pts, plain


def check_pairs(ofk, B, res, feas=False, pairs=2):
    sensors, out, rec, wts, pts, plain = res
    R = sensors[0, 7:16].reshape(3, 3)
    solved = 0
    for b in range(min(B, pairs)):
        n = int(out["counts"][b])
        w = None if wts is None else wts[b, :n]
        ref = jr.pair_joint(jr.NODE, pts[0][b, :n], pts[1][b, :n], out["status"][b, :n], sensors[b], JOINT["sigma_flow"], (JOINT["sigma_omega"],) * 3,
                            plain["records"][b], w=w, use_feas=feas, feas_T=-0.8)
        tag = f"B {B} pair {b}"
        assert ref["flag"] == 0 and plain["records"][b, 4] == 3, tag
        assert_joint_close(out["records"][b, 0:3], out["records"][b, 3], rec[b], ref, tag)
        vu = R @ (out["records"][b, 0:3] - np.cross(rec[b, 0:3], sensors[b, 16:19]))
        np.testing.assert_allclose(out["records"][b, 8:11], vu, rtol=0, atol=4e-16 * np.abs(vu).max() * 8, err_msg=tag)
        assert not np.array_equal(out["records"][b, 0:3], plain["records"][b, 0:3])
        solved += 1
    assert solved


def test_pairs_launch_forms_slices_and_overlap(pkg, ofk):
    """The same two pairs as batch 2 (a workgroup per pair) and batch 130 (a wave per pair), in one and two slices, with overlap on and
    off: records and joint records are the same bits; the records equal the reference joint solve of the downloaded points."""
    base = run_pairs(ofk, 2, JOINT)
    check_pairs(ofk, 2, base)
    for B, kw in ((130, {}), (130, dict(slices=2)), (2, dict(slices=2)), (130, dict(overlap=False)), (2, dict(overlap=False))):
        res = run_pairs(ofk, B, JOINT, **kw)
        for b in range(B):
            assert np.array_equal(bits(res[1]["records"][b]), bits(base[1]["records"][b % 2])), (B, kw, b)
            assert np.array_equal(bits(res[2][b]), bits(base[2][b % 2])), (B, kw, b)
    # the gyro error is what the joint solve takes out: closer to the renderer's truth than the plain solve
    truth = np.asarray(MOTION["v"])
    assert np.linalg.norm(base[1]["records"][0, :3] - truth) < np.linalg.norm(base[5]["records"][0, :3] - truth)
    print(f"pairs: largest deviation of (v, omega^) so far {SEEN['dev']:.3e}")


def test_pairs_all_axes_held_is_off(pkg, ofk):
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    prev, nxt, base = pair_frames(2)
    cfg = PipelineConfig(max_corners=CORNERS, quality=0.01, min_distance=6, block_size=5, win=15, max_level=2, max_count=20, eps=0.03)
    pipe = FlowPipeline(W, H, 2, cfg)
    try:
        pipe.upload(prev, nxt, pair_sensors(ofk, 2, base))
        plain = pipe.run()
        pipe.ctx.set_joint(sigma_flow=0.2, sigma_omega=0.0)
        out = pipe.run()
        rec = pipe.rotations()
    finally:
        pipe.close()
    for k in ("records", "prev_pts", "next_pts", "status", "err", "counts"):
        assert np.array_equal(bits(out[k]), bits(plain[k])), k
    assert np.all(rec[:, 10] == 0) and np.all(rec[:, 3:6] == 0) and np.all(rec[:, 21] > 0)


COMBOS = [
    pytest.param(dict(robust=dict(loss="huber", hypotheses=16, seed=5)), id="robust"),
    pytest.param(dict(gate=dict(fb="plain", fb_thr=0.5)), id="gate"),
    pytest.param(dict(seed="rotation"), id="seed"),
    pytest.param(dict(feas=True), id="feasibility"),
    pytest.param(dict(camera=dict(model="brown", fx=200.0, cx=80.0, cy=60.0, k=(-0.05, 0.01, 0.0, 0.0))), id="camera"),
    pytest.param(dict(rshutter=dict(mode="gyro", readout=0.5)), id="rolling-shutter"),
]


@pytest.mark.parametrize("kw", COMBOS)
def test_pairs_with_another_setting_on(pkg, ofk, kw):
    res = run_pairs(ofk, 2, JOINT, **kw)
    check_pairs(ofk, 2, res, feas=kw.get("feas", False))


def test_pairs_refusals_and_the_filter_step(pkg, ofk):
    from of_amd.pipeline import FlowPipeline, PipelineConfig, FilterModel
    prev, nxt, base = pair_frames(2)
    cfg = PipelineConfig(max_corners=CORNERS, quality=0.01, min_distance=6, block_size=5, win=15, max_level=2, max_count=20, eps=0.03)
    model = FilterModel.kf3()
    model.R = 1e-4 * np.eye(3); model.P0 = 1e-4 * np.eye(3)
    pipe = FlowPipeline(W, H, 2, cfg)
    try:
        pipe.ctx.filter_configure(model, 2)
        pipe.upload(prev, nxt, pair_sensors(ofk, 2, base))
        pipe.ctx.set_joint(**JOINT)
        pipe.ctx.set_cov(mode="propagate", sigma_flow=0.3)
        with pytest.raises(ofk.OfkError) as e:                   # the covariance takes omega as an input
            pipe.run()
        assert e.value.code == ofk.E_INVALID
        pipe.ctx.set_cov(None)
        out = pipe.run()
        pipe.ctx.pairs_filter_step(2, z_sign=-1.0, z_source=1)   # reads the rewritten records
        x, P = pipe.ctx.filter_state(2)
        rec = pipe.rotations()
    finally:
        pipe.close()
    assert np.all(rec[:, 10] == 0)
    for b in range(2):
        xp, Pp = eo.kf_predict(np.array(model.x0), np.array(model.P0), model.F, model.Q)
        xr, Pr = eo.kf_correct(xp, Pp, model.H, model.R, -out["records"][b, 8:11])
        np.testing.assert_allclose(x[b], xr, rtol=1e-9, atol=1e-15); np.testing.assert_allclose(P[b], Pr, rtol=1e-9, atol=1e-18)


# ---------------------------------------------------------------------------------------------------- stream steps
def stream_run(ofk, joint, fusion_name, T=3):
    """2 streams x T frames; per step what the device reported and what the reference needs (tests/second_stage_runs.py, which the
    tests of the declined second stage share)."""
    import second_stage_runs as ss
    steps, sensors, fusion = ss.stream_run(ofk, ("joint", joint) if joint is not None else None, fusion_name, T=T)
    for st in steps:
        st["joint"] = st["second"]
    return steps, sensors, fusion


@pytest.mark.parametrize("fusion_name", ("plain", "ekf6", "node", "replace"))
def test_stream_steps(pkg, ofk, fusion_name):
    off, _, _ = stream_run(ofk, None, fusion_name)
    steps, sensors, fusion = stream_run(ofk, JOINT, fusion_name)
    held, _, _ = stream_run(ofk, dict(sigma_flow=0.2, sigma_omega=0.0), fusion_name, T=2)
    for k in ("rec", "fused", "x", "P", "nxt", "keep"):          # all axes held: the bits of the setting off, the filter included
        if off[0][k] is not None:
            assert np.array_equal(bits(held[0][k]), bits(off[0][k])), k
    assert np.array_equal(bits(steps[0]["nxt"]), bits(off[0]["nxt"])) and np.array_equal(steps[0]["keep"], off[0]["keep"])
    for s in range(2):
        if fusion is not None and fusion.filter:
            xk, Pk = np.array(fusion.model.x0, np.float64), np.array(fusion.model.P0, np.float64)
        for k, st in enumerate(steps):
            n = int(st["n"][s])
            tag = f"{fusion_name} stream {s} step {k}"
            rec, jrec = st["rec"][s], st["joint"][s]
            use_imu = fusion is not None and fusion.use_imu
            nrm, om0 = (st["imu"][s, 15:18], st["imu"][s, 18:21]) if use_imu else (None, None)
            R = st["imu"][s, 6:15].reshape(3, 3) if use_imu else sensors[s, 7:16].reshape(3, 3)
            before = rec.copy(); before[0:4] = jrec[6:10]
            keepf = st["keep"][s, :n].astype(bool) if fusion is not None else None
            ref = jr.pair_joint(jr.NODE, st["old"][s, :n], st["nxt"][s, :n], st["keep"][s, :n], sensors[s], JOINT["sigma_flow"], (JOINT["sigma_omega"],) * 3,
                                before, keep=keepf, nrm=nrm, omega=om0, solved=fusion is None or rec[15] != 0)
            assert ref["flag"] == 0 and rec[4] == 3, tag
            assert_joint_close(rec[0:3], rec[3], jrec, ref, tag)
            vu = R @ (rec[0:3] - np.cross(jrec[0:3], sensors[s, 16:19]))
            np.testing.assert_allclose(rec[8:11], vu, rtol=0, atol=3e-15 * np.abs(vu).max(), err_msg=tag)
            if k == 0:
                assert not np.array_equal(rec[0:3], off[0]["rec"][s, 0:3]), tag
            if fusion is None:
                continue
            if fusion.filter:
                m = fusion.model
                xk, Pk = eo.kf_predict(xk, Pk, m.F, m.Q, m.B if m.nc else None, (st["dv"][s] if use_imu else sensors[s, 25:28]) if m.nc else None)
                z = fusion.z_sign * (rec[8:11] if fusion.z_source else rec[0:3])
                xk, Pk = eo.kf_correct(xk, Pk, m.H, m.R, z)
                fused = np.zeros(8); fused[:m.ns] = xk; fused[6] = np.trace(Pk); fused[7] = 1.0
                np.testing.assert_allclose(st["x"][s], xk, rtol=1e-9, atol=1e-15, err_msg=tag)
                np.testing.assert_allclose(st["P"][s], Pk, rtol=1e-9, atol=1e-18, err_msg=tag)
                np.testing.assert_allclose(st["fused"][s], fused, rtol=1e-9, atol=1e-15, err_msg=tag)
            else:
                assert np.array_equal(st["fused"][s, 0:3], rec[8:11]) and st["fused"][s, 7] == 1, tag
            if fusion.vel_overwrite:
                assert np.array_equal(st["imu_after"][s, 0:3], rec[8:11]), tag         # the joint v_uav, not the solve's
    print(f"{fusion_name}: largest deviation of (v, omega^) so far {SEEN['dev']:.3e}")


def test_stream_refusals(pkg, ofk):
    from of_amd.pipeline import FlowStream, PipelineConfig, FusionConfig
    fs = FlowStream(W, H, batch=1, cfg=PipelineConfig.of_module(), fusion=FusionConfig.of_module())
    try:
        fs.ctx.set_joint(**JOINT)
        prev, nxt, _ = pair_frames(1)
        fs.begin(prev)
        with pytest.raises(ofk.OfkError, match="sensor model"):
            fs.step_fused(nxt, ofk.make_sensors(1))
    finally:
        fs.close()
    cfg = PipelineConfig(max_corners=CORNERS, quality=0.01, min_distance=6, block_size=5, win=15, max_level=2, max_count=20, eps=0.03)
    fs = FlowStream(W, H, batch=1, cfg=cfg, fusion=FusionConfig.node())
    try:
        fs.ctx.set_joint(**JOINT)
        fs.ctx.set_cov(mode="propagate", sigma_flow=0.3)
        prev, nxt, _ = pair_frames(1)
        fs.begin(prev)
        with pytest.raises(ofk.OfkError, match="ofk_set_cov"):
            fs.step_fused(nxt, ofk.make_sensors(1))
    finally:
        fs.close()
