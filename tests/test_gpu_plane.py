"""GPU: the plane solve (ofk_set_plane / ofk_velocity_solve_plane) against tests/plane_reference.py.

(v, m^ = n^ / d^) of the device lie within TOL of the restatement's, in the measure of plane_reference.rel_dev: TOL is the tolerance
tests/test_plane_reference.py pins on the CPU (16 x the largest deviation of the restatement from a Gauss-Newton on stacked lstsq).
The residual sum of squares and the two objectives are held to RSS_TOL = 1e-10 relative under tests/test_gpu_joint.py's rule and
argument: stationary at the minimum, so only the rounding of a sum of at most 1025 f64 terms and the square of TOL reach them, plus
an absolute floor for exact fits, 3 m ((TOL + 8 eps) scale)^2 with `scale` the largest |sB X q|.  The record's eigenvalues,
covariances, predicted sigma and angle are held to REC_TOL = 1e-9 of their block's largest entry (rounding of about 2e-16 n cond stays
below 1e-10 at the conditions asserted here, COND_MAX; a wrong term is off by orders of magnitude more).  The last step's size (slot
16) is a difference of two iterates: it is held to 1e-6 relative plus 1e-11, the size rounding leaves of it.  The resident paths
feed the reference with the points, status and sensors the device downloaded; their image stages have their own suites."""
import numpy as np
import pytest

import plane_reference as pr
from oracle import estimation_oracle as eo
from plane_checks import PLANE, RSS_TOL, SEEN, assert_plane_close
from point_stage_helpers import bits
from test_plane_reference import TOL

pytestmark = pytest.mark.gpu


def batch3(n, **kw):
    sc = [pr.scene(n, 500 * n + b, **kw) for b in range(3)]
    return tuple(np.stack([s[k] for s in sc]) for k in range(7))


@pytest.mark.parametrize("n", pr.COUNTS)
def test_stage_entry(gpu_ctx, ofk, n):
    x, u, d, nrm, om, v, mt = batch3(n)
    t = np.array([[0.02, -0.01, 0.2]] * 3)
    mask = np.ones((3, n), np.uint8)
    if n > 8:
        mask[:, 4::3] = 0                                        # every third point from the fifth on is skipped
    for variant in (ofk.SOLVE_NODE, ofk.SOLVE_SIM):
        for name, prior in pr.PRIORS.items():
            for valid, lever in ((None, None), (mask, t)):
                plain = gpu_ctx.velocity_solve(variant, x, u, d=d, nrm=nrm, omega=om, valid=valid)
                before = gpu_ctx.velocity_solve(variant, x, u, d=d, nrm=nrm, omega=om, t=lever, valid=valid)        # what the plane kernel finds in `out`
                out, rec = gpu_ctx.velocity_solve_plane(variant, x, u, d=d, nrm=nrm, omega=om, t=lever, valid=valid, sigma_flow=pr.SIGMA_FLOW,
                                                        sigma_normal=prior)
                assert np.array_equal(bits(out[:, 4:8]), bits(plain[:, 4:8]))
                for b in range(3):
                    tag = f"n {n} variant {variant} prior {name} valid {valid is not None} problem {b}"
                    ref = pr.plane_solve(variant, x[b], u[b], d[b], nrm[b], om[b], pr.SIGMA_FLOW, prior, v_s=plain[b, :3], rss_s=plain[b, 3],
                                         rank=plain[b, 4], valid=None if valid is None else valid[b])
                    assert ref["flag"] == 0, tag
                    vdev = out[b, :3] + (np.cross(om[b], lever[b]) if lever is not None else 0.0)
                    ref["rec"][6:9] = before[b, :3]              # slots 6-8 hold out's fields as they were: v_s less omega x t
                    assert_plane_close(vdev, out[b, 3], rec[b], ref, tag)
    print(f"n {n}: largest deviation of (v, m^) so far {SEEN['dev']:.3e} (TOL {TOL:.2e})")


def test_stage_entry_with_the_robust_setting(gpu_ctx, ofk):
    n = 257
    x, u, d, nrm, om, v, mt = batch3(n, outliers=True)
    setting = ofk.robust_setting("tukey", hypotheses=32, seed=77)
    for variant in (ofk.SOLVE_NODE, ofk.SOLVE_SIM):
        out_r, w, st = gpu_ctx.velocity_solve_robust(variant, x, u, d=d, nrm=nrm, omega=om, robust=setting)
        assert np.any((w > 0) & (w < 1))
        out, rec = gpu_ctx.velocity_solve_plane(variant, x, u, d=d, nrm=nrm, omega=om, robust=setting, sigma_flow=pr.SIGMA_FLOW, sigma_normal=0.05)
        for b in range(3):
            ref = pr.plane_solve(variant, x[b], u[b], d[b], nrm[b], om[b], pr.SIGMA_FLOW, 0.05, v_s=out_r[b, :3], rss_s=out_r[b, 3], rank=out_r[b, 4],
                                 w=w[b])
            assert ref["flag"] == 0 and rec[b, 11] == np.count_nonzero(w[b] > 0)
            assert_plane_close(out[b, :3], out[b, 3], rec[b], ref, f"robust variant {variant} problem {b}")


def test_stage_entry_flags_and_the_held_prior(gpu_ctx, ofk):
    x, u, d, nrm, om, v, mt = batch3(20, noise=0.0)
    kw = dict(nrm=nrm, omega=om, sigma_flow=pr.SIGMA_FLOW)
    # flag 1: one point; d = 0; a NaN range among finite problems, which keep their bits
    plain = gpu_ctx.velocity_solve(ofk.SOLVE_NODE, x[:, :1], u[:, :1], d=d, nrm=nrm, omega=om)
    out, rec = gpu_ctx.velocity_solve_plane(ofk.SOLVE_NODE, x[:, :1], u[:, :1], d=d, **kw)
    assert np.array_equal(bits(out), bits(plain)) and np.all(rec[:, 10] == 1) and np.array_equal(rec[:, 0:3], nrm) and np.array_equal(rec[:, 3], d)
    assert np.all(rec[:, 11] == 1)
    good, grec = gpu_ctx.velocity_solve_plane(ofk.SOLVE_NODE, x, u, d=d, **kw)
    assert np.all(grec[:, 10] == 0)
    for bad in (0.0, np.nan):
        dd = d.copy(); dd[1] = bad
        plain = gpu_ctx.velocity_solve(ofk.SOLVE_NODE, x, u, d=dd, nrm=nrm, omega=om)
        out, rec = gpu_ctx.velocity_solve_plane(ofk.SOLVE_NODE, x, u, d=dd, **kw)
        assert rec[1, 10] == 1 and np.array_equal(bits(out[1]), bits(plain[1])) and np.all(rec[1, 4:6] == 0) and np.all(rec[1, 12:] == 0)
        for b in (0, 2):
            assert np.array_equal(bits(out[b]), bits(good[b])) and np.array_equal(bits(rec[b]), bits(grec[b])), (bad, b)
    # a normal at right angles to the beam: the gauge has nothing to hold
    side = np.broadcast_to(np.array([1.0, 0.0, 0.0]), (3, 3)).copy()
    plain = gpu_ctx.velocity_solve(ofk.SOLVE_SIM, x, u, d=d, nrm=side, omega=om)
    out, rec = gpu_ctx.velocity_solve_plane(ofk.SOLVE_SIM, x, u, d=d, nrm=side, omega=om, sigma_flow=pr.SIGMA_FLOW)
    assert np.all(rec[:, 10] == 1) and np.array_equal(bits(out), bits(plain))
    # exact flow: the truth comes back
    assert np.abs(good[:, :3] - v).max() <= 1e-12 and np.abs(grec[:, 0:3] / grec[:, 3:4] - mt).max() <= 1e-11
    # flag 2: a hover (the flow of v = 0 with noise: the solve's v is noise) - and the gate at the predicted sigma
    rng = np.random.default_rng(9)
    u0 = np.stack([eo.generate_test_data(x[b], np.zeros(3), om[b], d[b], nrm[b]) for b in range(3)]) + rng.normal(0, pr.SIGMA_FLOW, u.shape)
    plain = gpu_ctx.velocity_solve(ofk.SOLVE_NODE, x, u0, d=d, nrm=nrm, omega=om)
    out, rec = gpu_ctx.velocity_solve_plane(ofk.SOLVE_NODE, x, u0, d=d, **kw)
    assert np.all(plain[:, 4] == 3) and np.all(rec[:, 10] == 2) and np.array_equal(bits(out), bits(plain)) and np.array_equal(rec[:, 0:3], nrm)
    assert np.all(rec[:, 4:6] == 0) and np.all(rec[:, 14:26] == 0)
    x, u, d, nrm, om, v, mt = batch3(65)
    kw = dict(nrm=nrm, omega=om, sigma_flow=pr.SIGMA_FLOW)
    plain = gpu_ctx.velocity_solve(ofk.SOLVE_NODE, x, u, d=d, nrm=nrm, omega=om)
    full, frec = gpu_ctx.velocity_solve_plane(ofk.SOLVE_NODE, x, u, d=d, **kw)
    assert np.all(frec[:, 10] == 0) and np.all(frec[:, 14] > 0) and np.all(frec[:, 14] < 0.1)
    out, rec = gpu_ctx.velocity_solve_plane(ofk.SOLVE_NODE, x, u, d=d, sigma_max=frec[:, 14].min() * (1 - 1e-9), **kw)
    assert np.all(rec[:, 10] == 2) and np.array_equal(bits(out), bits(plain)) and np.array_equal(bits(rec[:, 12:14]), bits(frec[:, 12:14]))
    out, rec = gpu_ctx.velocity_solve_plane(ofk.SOLVE_NODE, x, u, d=d, sigma_max=np.inf, **kw)
    assert np.array_equal(bits(out), bits(full)) and np.array_equal(bits(rec), bits(frec))
    # a prior term that overflows: flag 1, out has the plain solve's bits, the record is the reference's to the bit.  1e-160: Lambda is
    # +inf and no walk is evaluated; 1e-153: Lambda is finite, the 2 x 2's determinant is not, the first objective stays in slot 26
    for variant in (ofk.SOLVE_NODE, ofk.SOLVE_SIM):
        pl = gpu_ctx.velocity_solve(variant, x, u, d=d, nrm=nrm, omega=om)
        for prior in (1e-160, 1e-153):
            out, rec = gpu_ctx.velocity_solve_plane(variant, x, u, d=d, sigma_normal=prior, **kw)
            assert np.array_equal(bits(out), bits(pl)), (variant, prior)
            for b in range(3):
                ref = pr.plane_solve(variant, x[b], u[b], d[b], nrm[b], om[b], pr.SIGMA_FLOW, prior, v_s=pl[b, :3], rss_s=pl[b, 3], rank=pl[b, 4])
                assert ref["flag"] == 1 and rec[b, 10] == 1 and rec[b, 11] == 65, (variant, prior, b, rec[b])
                assert not rec[b, 4:6].any() and not rec[b, 12:26].any() and not rec[b, 27:].any(), (variant, prior, b, rec[b])
                assert np.array_equal(bits(np.delete(rec[b], 26)), bits(np.delete(ref["rec"], 26))), (variant, prior, b, rec[b])
                assert (rec[b, 26] == 0) if prior == 1e-160 else abs(rec[b, 26] - ref["rec"][26]) <= RSS_TOL * ref["rec"][26], (variant, prior, b, rec[b, 26])
    # two points: rank 3 for v, a singular S with the tilt free (flag 2); three points are enough - against the reference
    x8, u8, d8, nrm8, om8, _, _ = (np.stack([pr.scene(8, 6 + b)[k] for b in range(3)]) for k in range(7))
    for count, want in ((2, 2), (3, 0)):
        pl = gpu_ctx.velocity_solve(ofk.SOLVE_NODE, x8[:, :count], u8[:, :count], d=d8, nrm=nrm8, omega=om8)
        out, rec = gpu_ctx.velocity_solve_plane(ofk.SOLVE_NODE, x8[:, :count], u8[:, :count], d=d8, nrm=nrm8, omega=om8, sigma_flow=pr.SIGMA_FLOW)
        assert np.all(pl[:, 4] == 3)
        for b in range(3):
            ref = pr.plane_solve(pr.NODE, x8[b, :count], u8[b, :count], d8[b], nrm8[b], om8[b], pr.SIGMA_FLOW, np.inf, v_s=pl[b, :3], rss_s=pl[b, 3],
                                 rank=pl[b, 4])
            assert ref["flag"] == want and rec[b, 11] == count, (count, b, ref["flag"])
            if want == 2:                                        # S is singular in every walk: which walk's rounding ends it is not pinned, the flag is
                assert np.array_equal(bits(out[b]), bits(pl[b])), (b, rec[b, 12:14])
            assert_plane_close(out[b, :3], out[b, 3], rec[b], ref, f"{count} points problem {b}")
    # held: the plain solve's bits
    plain_sim = gpu_ctx.velocity_solve(ofk.SOLVE_SIM, x, u, d=d, nrm=nrm, omega=om, t=om)
    out, rec = gpu_ctx.velocity_solve_plane(ofk.SOLVE_SIM, x, u, d=d, t=om, sigma_normal=0.0, **kw)
    assert np.array_equal(bits(out), bits(plain_sim)) and np.all(rec[:, 10] == 0) and np.all(rec[:, 4:6] == 0)
    assert np.allclose(rec[:, 0:3], nrm, rtol=0, atol=1e-15) and np.allclose(rec[:, 3], d, rtol=0, atol=1e-15)
    assert np.all(rec[:, 12:20] == 0) and np.all(rec[:, [20, 23, 25]] > 0) and np.array_equal(rec[:, 26], rec[:, 27])
    # iters: one step is not six
    one, orec = gpu_ctx.velocity_solve_plane(ofk.SOLVE_NODE, x, u, d=d, iters=1, **kw)
    assert np.all(orec[:, 10] == 0) and np.all(orec[:, 16] > 1e3 * frec[:, 16]) and not np.array_equal(one[:, :3], full[:, :3])
    for b in range(3):
        ref = pr.plane_solve(pr.NODE, x[b], u[b], d[b], nrm[b], om[b], pr.SIGMA_FLOW, np.inf, iters=1, v_s=plain[b, :3], rss_s=plain[b, 3],
                             rank=plain[b, 4])
        assert_plane_close(one[b, :3], one[b, 3], orec[b], ref, f"iters 1 problem {b}")
    # another beam: the gauge holds m.e
    e = np.array([0.0, 0.6, 0.8])
    out, rec = gpu_ctx.velocity_solve_plane(ofk.SOLVE_NODE, x, u, d=d, beam=e, **kw)
    assert np.all(rec[:, 10] == 0)
    np.testing.assert_allclose((rec[:, 0:3] / rec[:, 3:4]) @ e, (nrm @ e) / d, rtol=1e-14)


# ---------------------------------------------------------------------------------------------------- resident pairs
H, W, CORNERS = 120, 160, 64                                     # tests/test_gpu_cov.py's frame
SLOPE = np.radians(10.0)
GROUND = (np.sin(SLOPE) * 0.6, -np.sin(SLOPE) * 0.8, np.cos(SLOPE))      # what the frames show: a plane 10 degrees off the level one
MOTION = dict(v=(0.012, -0.009, 0.004), omega=(0.003, -0.002, 0.004), d=1.0, n=GROUND)
LEVEL = dict(d=1.0 / GROUND[2], normal=(0.0, 0.0, 1.0))          # what the sensors say: level ground at the range along the optical axis
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
    return ofk.make_sensors(B, omega=p0["omega"], rotation=R, offset=(0.02, -0.01, 0.2), scaling=p0["scaling"], cx=p0["cx"], cy=p0["cy"],
                            v_prior=p0["v"], **LEVEL)


def run_pairs(ofk, B, plane, slices=1, overlap=True, feas=False, robust=None, gate=None, seed=None, camera=None, rshutter=None):
    """A run with the setting off, one with it on, one with it off again.  Returns sensors, the run with it on, the plane records, the
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
            pipe.planes()                                        # nothing ran with the setting on yet
        pipe.ctx.set_plane(**plane)
        out = pipe.run()
        rec = pipe.planes()
        wts = pipe.ctx.robust_download(B)[0] if robust else None
        pts = pipe.ctx.camera_download(B) if camera else pipe.ctx.rs_download(B) if rshutter else (out["prev_pts"], out["next_pts"])
        pipe.ctx.set_plane(None)
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
    for b in range(min(B, pairs)):
        n = int(out["counts"][b])
        w = None if wts is None else wts[b, :n]
        ref = pr.pair_plane(pr.NODE, pts[0][b, :n], pts[1][b, :n], out["status"][b, :n], sensors[b], PLANE["sigma_flow"], PLANE["sigma_normal"],
                            plain["records"][b], w=w, use_feas=feas, feas_T=-0.8)
        tag = f"B {B} pair {b}"
        assert ref["flag"] == 0 and plain["records"][b, 4] == 3, (tag, ref["flag"], ref["rec"][12:15])
        assert_plane_close(out["records"][b, 0:3], out["records"][b, 3], rec[b], ref, tag)
        vu = R @ (out["records"][b, 0:3] - np.cross(sensors[b, 4:7], sensors[b, 16:19]))
        np.testing.assert_allclose(out["records"][b, 8:11], vu, rtol=0, atol=4e-16 * np.abs(vu).max() * 8, err_msg=tag)
        assert not np.array_equal(out["records"][b, 0:3], plain["records"][b, 0:3])


def test_pairs_launch_forms_slices_and_overlap(pkg, ofk):
    """The same two pairs as batch 2 (a workgroup per pair) and batch 130 (a wave per pair), in one and two slices (130 pairs in two
    slices: 65 per slice, the workgroup form again), with overlap on and off: records and plane records are the same bits; the records
    equal the reference plane solve of the downloaded points."""
    base = run_pairs(ofk, 2, PLANE)
    check_pairs(ofk, 2, base)
    for B, kw in ((130, {}), (130, dict(slices=2)), (2, dict(slices=2)), (130, dict(overlap=False)), (2, dict(overlap=False))):
        res = run_pairs(ofk, B, PLANE, **kw)
        for b in range(B):
            assert np.array_equal(bits(res[1]["records"][b]), bits(base[1]["records"][b % 2])), (B, kw, b)
            assert np.array_equal(bits(res[2][b]), bits(base[2][b % 2])), (B, kw, b)
    # the slope is what the plane solve takes out: closer to the renderer's truth than the plain solve, the normal closer to the ground's
    truth = np.asarray(MOTION["v"])
    for b in range(2):
        assert np.linalg.norm(base[1]["records"][b, :3] - truth) < np.linalg.norm(base[5]["records"][b, :3] - truth)
        assert base[2][b, 0:3] @ np.asarray(GROUND) > GROUND[2]
    print(f"pairs: largest deviation of (v, m^) so far {SEEN['dev']:.3e}")


def test_pairs_held_is_off(pkg, ofk):
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    prev, nxt, base = pair_frames(2)
    cfg = PipelineConfig(max_corners=CORNERS, quality=0.01, min_distance=6, block_size=5, win=15, max_level=2, max_count=20, eps=0.03)
    pipe = FlowPipeline(W, H, 2, cfg)
    try:
        pipe.upload(prev, nxt, pair_sensors(ofk, 2, base))
        plain = pipe.run()
        pipe.ctx.set_plane(sigma_flow=0.2, sigma_normal=0.0)
        out = pipe.run()
        rec = pipe.planes()
    finally:
        pipe.close()
    for k in ("records", "prev_pts", "next_pts", "status", "err", "counts"):
        assert np.array_equal(bits(out[k]), bits(plain[k])), k
    assert np.all(rec[:, 10] == 0) and np.all(rec[:, 4:6] == 0) and np.all(rec[:, 20] > 0) and np.array_equal(rec[:, 0:3], np.array([[0.0, 0.0, 1.0]] * 2))


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
    res = run_pairs(ofk, 2, PLANE, **kw)
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
        pipe.ctx.set_plane(**PLANE)
        pipe.ctx.set_cov(mode="propagate", sigma_flow=0.3)
        with pytest.raises(ofk.OfkError, match="ofk_set_cov") as e:                # the covariance takes the normal as an input
            pipe.run()
        assert e.value.code == ofk.E_INVALID
        pipe.ctx.set_cov(None)
        pipe.ctx.set_joint(sigma_flow=0.2, sigma_omega=1e-3)
        with pytest.raises(ofk.OfkError, match="ofk_set_joint") as e:              # so does the joint solve
            pipe.run()
        assert e.value.code == ofk.E_INVALID
        pipe.ctx.set_joint(None)
        out = pipe.run()
        pipe.ctx.pairs_filter_step(2, z_sign=-1.0, z_source=1)   # reads the rewritten records
        x, P = pipe.ctx.filter_state(2)
        rec = pipe.planes()
    finally:
        pipe.close()
    assert np.all(rec[:, 10] == 0)
    for b in range(2):
        xp, Pp = eo.kf_predict(np.array(model.x0), np.array(model.P0), model.F, model.Q)
        xr, Pr = eo.kf_correct(xp, Pp, model.H, model.R, -out["records"][b, 8:11])
        np.testing.assert_allclose(x[b], xr, rtol=1e-9, atol=1e-15); np.testing.assert_allclose(P[b], Pr, rtol=1e-9, atol=1e-18)
    cfg = PipelineConfig.of_module()
    pipe = FlowPipeline(W, H, 2, cfg)
    try:
        pipe.upload(prev, nxt, pair_sensors(ofk, 2, base))
        pipe.ctx.set_plane(**PLANE)
        with pytest.raises(ofk.OfkError) as e:                   # OFK_SOLVE_OFMODULE: a pairs run takes NODE and SIM alone, setting or not
            pipe.run()
        assert e.value.code == ofk.E_INVALID
    finally:
        pipe.close()


# ---------------------------------------------------------------------------------------------------- stream steps
def stream_run(ofk, plane, fusion_name, T=4, then_off=False):
    """2 streams x T frames, that is T - 1 steps (the default: three); per step what the device reported and what the reference needs.  then_off: the setting is switched off
    again before the first frame."""
    from of_amd import synth
    from of_amd.pipeline import FlowStream, PipelineConfig, FusionConfig, FilterModel
    from stream_oracle import imu_messages
    B = 2
    if "stream" not in _frames:
        seqs = [synth.render_sequence(H, W, 7400 + s, 4, margin=64, **MOTION) for s in range(B)]
        _frames["stream"] = (np.stack([s[0] for s in seqs]), seqs[0][1])
    frames, info = _frames["stream"]
    cfg = PipelineConfig(max_corners=CORNERS, quality=0.01, min_distance=6, block_size=5, win=15, max_level=2, max_count=20, eps=0.03)
    if fusion_name == "ekf6":
        fusion = FusionConfig.ekf6(r=1e-4, p0=1e-4)
    elif fusion_name == "node":
        fusion = FusionConfig.node()
    elif fusion_name == "replace":
        model = FilterModel.kf3()
        model.R = 1e-4 * np.eye(3); model.P0 = 1e-4 * np.eye(3)
        fusion = FusionConfig(filter=True, z_sign=-1.0, z_source=1, redetect_replace=True, model=model)
    else:
        fusion = None
    sensors = ofk.make_sensors(B, omega=info["omega"], offset=(0.02, -0.01, 0.2), scaling=info["scaling"], cx=info["cx"], cy=info["cy"],
                               v_prior=MOTION["v"], **LEVEL)
    fs = FlowStream(W, H, batch=B, cfg=cfg, min_features=10, mask_radius=8, fusion=fusion)
    steps = []
    try:
        if plane is not None:
            fs.ctx.set_plane(**plane)
        if then_off:
            fs.ctx.set_plane(None)
            plane = None
        tracks, counts = fs.begin(frames[:, 0])
        rng = np.random.default_rng(31)
        for t in range(1, T):
            imu = dv = None
            if fusion is not None and fusion.use_imu:
                msgs = np.stack([imu_messages(rng, 0.1 * t + 10 * s, 3, rate=np.asarray(info["omega"])) for s in range(B)])
                fs.push_imu(msgs)
                imu, dv = fs.ctx.imu_state(B)
            old_tracks, old_counts = tracks.copy(), counts.copy()
            if fusion is None:
                rec, tracks, counts = fs.step(frames[:, t], sensors)
                fused = x = P = None
            else:
                rec, fused, tracks, counts = fs.step_fused(frames[:, t], sensors)
                x, P = fs.ctx.filter_state(B) if fusion.filter else (None, None)
            nxt, keep = fs.ctx.stream_last_points(CORNERS)
            imu_after = fs.ctx.imu_state(B)[0] if fusion is not None and fusion.use_imu else None
            steps.append(dict(rec=rec, fused=fused, old=old_tracks, n=old_counts, nxt=nxt, keep=keep, imu=imu, dv=dv, x=x, P=P, imu_after=imu_after,
                              plane=fs.planes() if plane is not None else None))
    finally:
        fs.close()
    return steps, sensors, fusion


@pytest.mark.parametrize("fusion_name", ("plain", "ekf6", "node", "replace"))
def test_stream_steps(pkg, ofk, fusion_name):
    off, _, _ = stream_run(ofk, None, fusion_name)
    steps, sensors, fusion = stream_run(ofk, PLANE, fusion_name)
    held, _, _ = stream_run(ofk, dict(sigma_flow=0.2, sigma_normal=0.0), fusion_name, T=2)
    again, _, _ = stream_run(ofk, PLANE, fusion_name, T=2, then_off=True)
    for k in ("rec", "fused", "x", "P", "nxt", "keep", "imu_after"):                  # switched off: a context that never saw the setting
        if off[0][k] is not None:
            assert np.array_equal(bits(again[0][k]), bits(off[0][k])), k
    for k in ("rec", "fused", "x", "P", "nxt", "keep"):          # held: the bits of the setting off, the filter included
        if off[0][k] is not None:
            assert np.array_equal(bits(held[0][k]), bits(off[0][k])), k
    assert np.array_equal(bits(steps[0]["nxt"]), bits(off[0]["nxt"])) and np.array_equal(steps[0]["keep"], off[0]["keep"])
    rewritten = 0
    for s in range(2):
        if fusion is not None and fusion.filter:
            xk, Pk = np.array(fusion.model.x0, np.float64), np.array(fusion.model.P0, np.float64)
        for k, st in enumerate(steps):
            n = int(st["n"][s])
            tag = f"{fusion_name} stream {s} step {k}"
            rec, prec = st["rec"][s], st["plane"][s]
            use_imu = fusion is not None and fusion.use_imu
            nrm, om = (st["imu"][s, 15:18], st["imu"][s, 18:21]) if use_imu else (None, sensors[s, 4:7])
            R = st["imu"][s, 6:15].reshape(3, 3) if use_imu else sensors[s, 7:16].reshape(3, 3)
            before = rec.copy(); before[0:4] = prec[6:10]
            keepf = st["keep"][s, :n].astype(bool) if fusion is not None else None
            ref = pr.pair_plane(pr.NODE, st["old"][s, :n], st["nxt"][s, :n], st["keep"][s, :n], sensors[s], PLANE["sigma_flow"], PLANE["sigma_normal"],
                                before, keep=keepf, nrm=nrm, omega=om if use_imu else None, solved=fusion is None or rec[15] != 0)
            assert rec[4] == 3, tag
            assert_plane_close(rec[0:3], rec[3], prec, ref, tag)
            if ref["flag"] == 0:
                rewritten += 1
                vu = R @ (rec[0:3] - np.cross(om, sensors[s, 16:19]))
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
                assert np.array_equal(st["imu_after"][s, 0:3], rec[8:11]), tag         # the refined v_uav where the record was rewritten
    assert len(steps) == 3 and rewritten                         # three steps; the streams are not all flagged
    print(f"{fusion_name}: {rewritten} of {2 * len(steps)} steps rewritten, largest deviation of (v, m^) so far {SEEN['dev']:.3e}")


def test_stream_refusals(pkg, ofk):
    from of_amd.pipeline import FlowStream, PipelineConfig, FusionConfig
    fs = FlowStream(W, H, batch=1, cfg=PipelineConfig.of_module(), fusion=FusionConfig.of_module())
    try:
        fs.ctx.set_plane(**PLANE)
        prev, nxt, _ = pair_frames(1)
        fs.begin(prev)
        with pytest.raises(ofk.OfkError, match="sensor model"):
            fs.step_fused(nxt, ofk.make_sensors(1))
    finally:
        fs.close()
    cfg = PipelineConfig(max_corners=CORNERS, quality=0.01, min_distance=6, block_size=5, win=15, max_level=2, max_count=20, eps=0.03)
    for other, name in ((lambda c: c.set_cov(mode="propagate", sigma_flow=0.3), "ofk_set_cov"),
                        (lambda c: c.set_joint(sigma_flow=0.2, sigma_omega=1e-3), "ofk_set_joint")):
        fs = FlowStream(W, H, batch=1, cfg=cfg, fusion=FusionConfig.node())
        try:
            fs.ctx.set_plane(**PLANE)
            other(fs.ctx)
            prev, nxt, _ = pair_frames(1)
            fs.begin(prev)
            with pytest.raises(ofk.OfkError, match=name):
                fs.step_fused(nxt, ofk.make_sensors(1))
        finally:
            fs.close()
