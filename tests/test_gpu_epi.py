"""GPU: the epipolar solve (ofk_set_epipolar / ofk_velocity_solve_epipolar) against tests/epi_reference.py.

(t^, s) of the device lie within TOL of the restatement's, in the measure of epi_reference.rel_dev: TOL is the tolerance
tests/test_epi_reference.py pins on the CPU (16 x the largest deviation of the restatement from the independent route).  The point
rows are held to TOL in the measure of epi_reference.rows_dev: rho_i and |b_i| relative to the largest of the problem, r_i relative
to the largest derotated flow |a_i| (r is a difference of flow-sized terms; where the fit is exact it is rounding alone); the point
flags must agree.  The record is held to REC_TOL = 1e-9 of its slot group's scale (epi_reference.record_scale), tests/test_gpu_cov.py's
bound with its argument: rounding of about 2e-16 n cond stays far below, a wrong term is off by orders of magnitude.  The resident
paths feed the reference with the points, status and sensors the device downloaded; their image stages have their own suites."""
import numpy as np
import pytest

import epi_reference as er
from oracle import estimation_oracle as eo
from point_stage_helpers import bits
from test_epi_reference import TOL

pytestmark = pytest.mark.gpu

REC_TOL = 1e-9
SEEN = dict(dev=0.0, rows=0.0, r=0.0)
GPU_COUNTS = (3, 64, 65, 257, 1025)


def assert_epi_close(v, rss, rec, rows, ref, tag):
    """The device's v, field 3, record and point rows against epi_solve's dict."""
    assert rec[10] == ref["flag"], (tag, "flag", rec[10], ref["flag"])
    assert rec[11] == ref["rec"][11] and rec[31] == 0, tag
    assert np.array_equal(rec[6:10], ref["rec"][6:10]), (tag, "the solve's v and residual before")
    if ref["flag"] != 0:
        assert np.array_equal(v, ref["v"]) and rss == ref["rss"], (tag, "the record is untouched")
        assert not rows.any(), (tag, "rows of a flagged problem are zero")
        assert rec[3] == 0 and np.all(rec[24:31] == 0), tag
        if ref["flag"] == 1:
            assert np.all(np.delete(rec, [6, 7, 8, 9, 10, 11]) == 0), tag
        return
    assert np.array_equal(rec[12:14], ref["rec"][12:14]), (tag, "anchor and negative counts", rec[12:14], ref["rec"][12:14])
    dev = er.rel_dev(rec[0:3], rec[3], ref["t"], ref["s"])
    SEEN["dev"] = max(SEEN["dev"], dev)
    assert dev <= TOL, (tag, dev)
    np.testing.assert_allclose(v, rec[3] * rec[0:3], rtol=0, atol=4 * er.EPS * rec[3], err_msg=tag)
    d_rho, d_r = er.rows_dev(rows, ref["rows"], ref["a_max"])
    SEEN["rows"] = max(SEEN["rows"], d_rho); SEEN["r"] = max(SEEN["r"], d_r)
    assert d_rho <= TOL and d_r <= TOL, (tag, "rows", d_rho, d_r)
    assert rss == rec[5], tag
    sc = er.record_scale(ref["rec"])
    err = np.abs(rec - ref["rec"]) / sc
    assert err.max() <= REC_TOL, (tag, int(err.argmax()), rec[err.argmax()], ref["rec"][err.argmax()])


def batch3(n, weights=False):
    cs = [case_seeded(n, b, weights) for b in range(3)]
    return tuple(np.stack([c[k] for c in cs]) for k in range(7)), cs[0][7]


def case_seeded(n, b, weights):
    x, u, d, nrm, om, v, rho = er.scene(n, 500 * n + b, kind="canopy" if n >= 8 else "flat", outliers=weights)
    kw = dict(anchor=er.FOOT, anchor_min=5) if n >= 8 else dict(anchor=np.inf, anchor_min=1)
    return x, u, d, nrm, om, v, rho, kw


@pytest.mark.parametrize("n", GPU_COUNTS)
def test_stage_entry(gpu_ctx, ofk, n):
    (x, u, d, nrm, om, v, rho), kw = batch3(n)
    t = np.array([[0.02, -0.01, 0.2]] * 3)
    mask = np.ones((3, n), np.uint8)
    if n > 8:
        mask[:, 9::3] = 0                                        # every third point from the tenth on is skipped
    for variant in (ofk.SOLVE_NODE, ofk.SOLVE_SIM):
        for valid, lever in ((None, None), (mask, t)):
            plain = gpu_ctx.velocity_solve(variant, x, u, d=d, nrm=nrm, omega=om, valid=valid)
            before = gpu_ctx.velocity_solve(variant, x, u, d=d, nrm=nrm, omega=om, t=lever, valid=valid)      # what the kernel finds in `out`
            out, rec, pts = gpu_ctx.velocity_solve_epipolar(variant, x, u, d=d, nrm=nrm, omega=om, t=lever, valid=valid, sigma_max=np.inf, **kw)
            assert np.array_equal(bits(out[:, 4:8]), bits(plain[:, 4:8]))
            for b in range(3):
                tag = f"n {n} variant {variant} valid {valid is not None} problem {b}"
                ref = er.epi_solve(x[b], u[b], d[b], nrm[b], om[b], v_s=before[b, :3], rss_s=before[b, 3], valid=None if valid is None else valid[b], **kw)
                assert ref["flag"] == 0, tag
                vdev = out[b, :3] + (np.cross(om[b], lever[b]) if lever is not None else 0.0)
                assert_epi_close(vdev, out[b, 3], rec[b], pts[b], ref, tag)
    print(f"n {n}: largest deviation of (t^, s) so far {SEEN['dev']:.3e}, of the rows {SEEN['rows']:.3e} / {SEEN['r']:.3e} (TOL {TOL:.2e})")


def test_stage_entry_with_the_robust_setting(gpu_ctx, ofk):
    n = 257
    (x, u, d, nrm, om, v, rho), kw = batch3(n, weights=True)
    setting = ofk.robust_setting("tukey", hypotheses=32, seed=77)
    out_r, w, st = gpu_ctx.velocity_solve_robust(ofk.SOLVE_NODE, x, u, d=d, nrm=nrm, omega=om, robust=setting)
    assert np.any((w > 0) & (w < 1))                             # real weights: the two modes solve different problems
    for mode, name in ((er.W_ONE, "one"), (er.W_ROBUST, "robust")):
        out, rec, pts = gpu_ctx.velocity_solve_epipolar(ofk.SOLVE_NODE, x, u, d=d, nrm=nrm, omega=om, robust=setting, weights=name, sigma_max=np.inf, **kw)
        for b in range(3):
            ref = er.epi_solve(x[b], u[b], d[b], nrm[b], om[b], v_s=out_r[b, :3], rss_s=out_r[b, 3], w=w[b], weights=mode, **kw)
            assert ref["flag"] == 0 and rec[b, 11] == (np.count_nonzero(w[b] > 0) if mode else n)
            assert_epi_close(out[b, :3], out[b, 3], rec[b], pts[b], ref, f"robust weights {name} problem {b}")


def test_stage_entry_flags_return_the_solve_bits(gpu_ctx, ofk):
    (x, u, d, nrm, om, v, rho), kw = batch3(65)
    base = dict(nrm=nrm, omega=om, sigma_max=np.inf, **kw)
    good, grec, gpts = gpu_ctx.velocity_solve_epipolar(ofk.SOLVE_NODE, x, u, d=d, **base)
    assert np.all(grec[:, 10] == 0)

    def flagged(flag, xx, uu, dd=d, **over):
        args = dict(base, **over)
        plain = gpu_ctx.velocity_solve(ofk.SOLVE_NODE, xx, uu, d=dd, nrm=args["nrm"], omega=args["omega"])
        out, rec, pts = gpu_ctx.velocity_solve_epipolar(ofk.SOLVE_NODE, xx, uu, d=dd, **args)
        assert np.array_equal(bits(out), bits(plain)), (flag, over)
        assert np.all(rec[:, 10] == flag), (flag, over, rec[:, 10])
        assert not pts.any() and np.array_equal(bits(rec[:, 6:10]), bits(plain[:, 0:4]))
        return rec
    for few in (1, 2):                                           # flag 1: one or two points
        rec = flagged(1, x[:, :few], u[:, :few], anchor=np.inf, anchor_min=1)
        assert np.all(rec[:, 11] == few) and np.all(np.delete(rec, [6, 7, 8, 9, 10, 11], 1) == 0)
        pl = gpu_ctx.velocity_solve(ofk.SOLVE_NODE, x[:, :few], u[:, :few], d=d, nrm=nrm, omega=om)
        for b in range(3):                                       # two points: rank 3 for the plain solve, no direction for this one - the reference's record
            ref = er.epi_solve(x[b, :few], u[b, :few], d[b], nrm[b], om[b], anchor=np.inf, anchor_min=1, v_s=pl[b, :3], rss_s=pl[b, 3])
            assert ref["flag"] == 1 and pl[b, 4] == (3 if few == 2 else 2) and np.array_equal(bits(rec[b]), bits(ref["rec"])), (few, b, rec[b])
    flagged(1, x, u, beam=(1.0, 0.0, 0.0))                       # e_z == 0
    flagged(1, x, u, nrm=np.array([[1.0, 0.0, 0.0]] * 3))        # n0.e == 0
    for bad in (0.0, np.nan):                                    # d0 = 0; a NaN range among finite problems, which keep their bits
        dd = d.copy(); dd[1] = bad
        plain = gpu_ctx.velocity_solve(ofk.SOLVE_NODE, x, u, d=dd, nrm=nrm, omega=om)
        out, rec, pts = gpu_ctx.velocity_solve_epipolar(ofk.SOLVE_NODE, x, u, d=dd, **base)
        assert rec[1, 10] == 1 and np.array_equal(bits(out[1]), bits(plain[1])) and not pts[1].any()
        for b in (0, 2):
            assert np.array_equal(bits(out[b]), bits(good[b])) and np.array_equal(bits(rec[b]), bits(grec[b])) and np.array_equal(bits(pts[b]), bits(gpts[b]))
    # flag 2: a hover, at the default gate
    hov = [er.scene(65, 500 * 65 + b, v=(0.0, 0.0, 0.0)) for b in range(3)]
    rec = flagged(2, np.stack([h[0] for h in hov]), np.stack([h[1] for h in hov]), sigma_max=ofk.EPI_SIGMA_MAX)
    assert np.all(rec[:, 17] > ofk.EPI_SIGMA_MAX) and np.all(rec[:, 3] == 0) and np.all(rec[:, 18:31] == 0)
    assert np.allclose(np.linalg.norm(rec[:, 0:3], axis=1), 1.0, rtol=0, atol=1e-14)
    # flag 3: an empty anchor; anchor_min not met
    rec = flagged(3, x, u, anchor=1e-6)
    assert np.all(rec[:, 12] == 0) and np.all(rec[:, 24:31] == 0) and np.all(rec[:, 18] != 0)
    na = int(grec[:, 12].min())
    assert np.all(gpu_ctx.velocity_solve_epipolar(ofk.SOLVE_NODE, x, u, d=d, **dict(base, anchor_min=na))[1][:, 10] == 0)
    flagged(3, x, u, anchor_min=int(grec[:, 12].max()) + 1)
    # exact flow over arbitrary depths: the truth comes back, every rho_i with it
    ex = [er.scene(65, 7 + b, noise=0.0) for b in range(3)]
    xe = np.stack([e[0] for e in ex]); ue = np.stack([e[1] for e in ex]); re = np.stack([e[6] for e in ex])
    out, rec, pts = gpu_ctx.velocity_solve_epipolar(ofk.SOLVE_NODE, xe, ue, d=d, **base)
    assert np.all(rec[:, 10] == 0) and np.abs(out[:, :3] - v).max() <= 1e-11 * np.linalg.norm(v[0]) and np.abs(pts[:, :, 0] / re - 1).max() <= 1e-11
    assert np.all(rec[:, 16] <= 1e-24 * rec[:, 14])
    # a point whose flow runs against the rest: point flag 2, counted in slot 13
    u2 = u.copy(); u2[0, 40] = er.flow(x[0, 40:41], v[0], om[0], -rho[0, 40:41])[0]
    out, rec, pts = gpu_ctx.velocity_solve_epipolar(ofk.SOLVE_NODE, x, u2, d=d, **base)
    assert rec[0, 10] == 0 and rec[0, 13] == 1 and pts[0, 40, 3] == 2 and pts[0, 40, 0] < 0 and np.all(np.delete(pts[0, :, 3], 40) == 0)
    # the mirrored motion: t^ follows the flow
    um = np.stack([er.flow(x[b], -v[b], om[b], rho[b]) for b in range(3)])
    out, rec, pts = gpu_ctx.velocity_solve_epipolar(ofk.SOLVE_NODE, x, um, d=d, **base)
    assert np.all(rec[:, 10] == 0) and np.abs(out[:, :3] + v).max() <= 1e-11 and np.all(pts[:, :, 0] > 0)


# ---------------------------------------------------------------------------------------------------- resident pairs
H, W, CORNERS = 120, 160, 64                                     # tests/test_gpu_joint.py's frame
MOTION = dict(v=(0.02, -0.015, 0.004), omega=(0.003, -0.002, 0.004), d=1.0)
EPI = dict(anchor=60.0, anchor_min=5, sigma_max=np.inf)          # 64 corners at 3 px of flow: the default gate would stop some pairs
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
    return ofk.make_sensors(B, d=p0["d"], normal=p0["n"], omega=p0["omega"], rotation=R, offset=(0.02, -0.01, 0.2),
                            scaling=p0["scaling"], cx=p0["cx"], cy=p0["cy"], v_prior=p0["v"])


def run_pairs(ofk, B, epi, slices=1, overlap=True, feas=False, robust=None, gate=None, seed=None, camera=None, rshutter=None, finite=None):
    """A run with the setting off, one with it on, one with it off again.  Returns sensors, the run with it on, the epipolar records and
    point rows, the robust weights, the points the solve stage read and the run with the setting off."""
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
        if finite:
            pipe.ctx.set_finite_motion(**finite)
        pipe.upload(prev, nxt, sensors)
        plain = pipe.run()
        with pytest.raises(ofk.OfkError):
            pipe.structure()                                     # nothing ran with the setting on yet
        pipe.ctx.set_epipolar(**epi)
        out = pipe.run()
        rec, rows = pipe.structure()
        wts = pipe.ctx.robust_download(B)[0] if robust else None
        pts = (pipe.ctx.finite_download(B) if finite else pipe.ctx.camera_download(B) if camera else pipe.ctx.rs_download(B) if rshutter
               else (out["prev_pts"], out["next_pts"]))
        pipe.ctx.set_epipolar(None)
        again = pipe.run()
    finally:
        pipe.close()
    for k in ("prev_pts", "next_pts", "status", "err", "counts"):                  # the image side: the setting changes none
        assert np.array_equal(bits(out[k]), bits(plain[k])), k
    for k in ("records", "prev_pts", "next_pts", "status", "err", "counts"):       # switched off: the bits of a context that never had it
        assert np.array_equal(bits(again[k]), bits(plain[k])), k
    keep = [4, 5, 6, 7, 11, 12, 13, 14, 15]
    assert np.array_equal(bits(out["records"][:, keep]), bits(plain["records"][:, keep]))
    return sensors, out, (rec, rows), wts, pts, plain


def check_pairs(ofk, B, res, epi, feas=False, pairs=2):
    sensors, out, (rec, rows), wts, pts, plain = res
    R = sensors[0, 7:16].reshape(3, 3)
    for b in range(min(B, pairs)):
        n = int(out["counts"][b])
        w = None if wts is None else wts[b, :n]
        ref = er.pair_epi(pts[0][b, :n], pts[1][b, :n], out["status"][b, :n], sensors[b], plain["records"][b], anchor_px=epi["anchor"],
                          anchor_min=epi["anchor_min"], sigma_max=epi["sigma_max"], weights=er.W_ROBUST if epi.get("weights") == "robust" else er.W_ONE,
                          w=w, use_feas=feas, feas_T=-0.8)
        tag = f"B {B} pair {b}"
        assert ref["flag"] == 0, (tag, ref["flag"], ref["rec"][11:14], ref["pred"])
        assert_epi_close(out["records"][b, 0:3], out["records"][b, 3], rec[b], rows[b, :n], ref, tag)
        assert np.all(rows[b, n:, 3] == 1) and not rows[b, n:, :3].any(), tag          # past the pair's count: not kept
        vu = R @ (out["records"][b, 0:3] - np.cross(sensors[b, 4:7], sensors[b, 16:19]))
        np.testing.assert_allclose(out["records"][b, 8:11], vu, rtol=0, atol=4e-16 * np.abs(vu).max() * 8, err_msg=tag)
        assert not np.array_equal(out["records"][b, 0:3], plain["records"][b, 0:3])


def test_pairs_launch_forms_slices_and_overlap(pkg, ofk):
    """The same two pairs as batch 2 (a workgroup per pair) and batch 130 (a wave per pair), in one and two slices, with overlap on and
    off: records, epipolar records and point rows are the same bits; they equal the reference solve of the downloaded points."""
    base = run_pairs(ofk, 2, EPI)
    check_pairs(ofk, 2, base, EPI)
    for B, kw in ((130, {}), (130, dict(slices=2)), (2, dict(slices=2)), (130, dict(overlap=False)), (2, dict(overlap=False))):
        res = run_pairs(ofk, B, EPI, **kw)
        for b in range(B):
            assert np.array_equal(bits(res[1]["records"][b]), bits(base[1]["records"][b % 2])), (B, kw, b)
            assert np.array_equal(bits(res[2][0][b]), bits(base[2][0][b % 2])), (B, kw, b)
            assert np.array_equal(bits(res[2][1][b]), bits(base[2][1][b % 2])), (B, kw, b)
    truth = np.asarray(MOTION["v"])
    for b in range(2):
        e = np.linalg.norm(base[1]["records"][b, :3] - truth) / np.linalg.norm(truth)
        print(f"pair {b}: epipolar v off by {e:.4f}, plain by {np.linalg.norm(base[5]['records'][b, :3] - truth) / np.linalg.norm(truth):.4f}")
        assert e < 0.1
    print(f"pairs: largest deviation of (t^, s) so far {SEEN['dev']:.3e}, of the rows {SEEN['rows']:.3e} / {SEEN['r']:.3e}")


def test_setting_off_is_a_context_that_never_saw_it(pkg, ofk):
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    prev, nxt, base = pair_frames(2)
    cfg = PipelineConfig(max_corners=CORNERS, quality=0.01, min_distance=6, block_size=5, win=15, max_level=2, max_count=20, eps=0.03)
    outs = []
    for touch in (False, True):
        pipe = FlowPipeline(W, H, 2, cfg)
        try:
            if touch:
                pipe.ctx.set_epipolar(**EPI); pipe.ctx.set_epipolar(None)
            pipe.upload(prev, nxt, pair_sensors(ofk, 2, base))
            outs.append(pipe.run())
            with pytest.raises(ofk.OfkError) as e:
                pipe.structure()
            assert e.value.code == ofk.E_INVALID
        finally:
            pipe.close()
    for k in ("records", "prev_pts", "next_pts", "status", "err", "counts"):
        assert np.array_equal(bits(outs[0][k]), bits(outs[1][k])), k


COMBOS = [
    pytest.param(dict(robust=dict(loss="huber", hypotheses=16, seed=5)), {}, id="robust-one"),
    pytest.param(dict(robust=dict(loss="tukey", hypotheses=16, seed=5)), dict(weights="robust"), id="robust-robust"),
    pytest.param(dict(gate=dict(fb="plain", fb_thr=0.5)), {}, id="gate"),
    pytest.param(dict(seed="rotation"), {}, id="seed"),
    pytest.param(dict(feas=True), {}, id="feasibility"),
    pytest.param(dict(camera=dict(model="brown", fx=200.0, cx=80.0, cy=60.0, k=(-0.05, 0.01, 0.0, 0.0))), {}, id="camera"),
    pytest.param(dict(rshutter=dict(mode="gyro", readout=0.5)), {}, id="rolling-shutter"),
    pytest.param(dict(finite=dict(mode="exact")), {}, id="finite-motion"),
]


@pytest.mark.parametrize("kw,over", COMBOS)
def test_pairs_with_another_setting_on(pkg, ofk, kw, over):
    epi = dict(EPI, **over)
    res = run_pairs(ofk, 2, epi, **kw)
    check_pairs(ofk, 2, res, epi, feas=kw.get("feas", False))


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
        pipe.ctx.set_epipolar(**EPI)
        for name, on, off in (("ofk_set_cov", lambda: pipe.ctx.set_cov(mode="propagate", sigma_flow=0.3), lambda: pipe.ctx.set_cov(None)),
                              ("ofk_set_joint", lambda: pipe.ctx.set_joint(sigma_flow=0.2), lambda: pipe.ctx.set_joint(None)),
                              ("ofk_set_plane", lambda: pipe.ctx.set_plane(sigma_flow=0.2), lambda: pipe.ctx.set_plane(None))):
            on()
            with pytest.raises(ofk.OfkError, match=name) as e:   # all three rest on the plane
                pipe.run()
            assert e.value.code == ofk.E_INVALID
            off()
        out = pipe.run()
        pipe.ctx.pairs_filter_step(2, z_sign=-1.0, z_source=1)   # reads the rewritten records
        x, P = pipe.ctx.filter_state(2)
        rec, rows = pipe.structure()
    finally:
        pipe.close()
    assert np.all(rec[:, 10] == 0)
    for b in range(2):
        xp, Pp = eo.kf_predict(np.array(model.x0), np.array(model.P0), model.F, model.Q)
        xr, Pr = eo.kf_correct(xp, Pp, model.H, model.R, -out["records"][b, 8:11])
        np.testing.assert_allclose(x[b], xr, rtol=1e-9, atol=1e-15); np.testing.assert_allclose(P[b], Pr, rtol=1e-9, atol=1e-18)


# ---------------------------------------------------------------------------------------------------- stream steps
def stream_run(ofk, epi, fusion_name, T=3):
    """2 streams x T frames; per step what the device reported and what the reference needs."""
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
    sensors = ofk.make_sensors(B, d=info["d"], normal=info["n"], omega=info["omega"], offset=(0.02, -0.01, 0.2),
                               scaling=info["scaling"], cx=info["cx"], cy=info["cy"], v_prior=MOTION["v"])
    fs = FlowStream(W, H, batch=B, cfg=cfg, min_features=10, mask_radius=8, fusion=fusion)
    steps = []
    try:
        if epi is not None:
            fs.ctx.set_epipolar(**epi)
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
                              epi=fs.structure() if epi is not None else None))
    finally:
        fs.close()
    return steps, sensors, fusion


@pytest.mark.parametrize("fusion_name", ("plain", "ekf6", "node", "replace"))
def test_stream_steps(pkg, ofk, fusion_name):
    off, _, _ = stream_run(ofk, None, fusion_name, T=2)
    steps, sensors, fusion = stream_run(ofk, EPI, fusion_name)
    assert np.array_equal(bits(steps[0]["nxt"]), bits(off[0]["nxt"])) and np.array_equal(steps[0]["keep"], off[0]["keep"])
    for s in range(2):
        if fusion is not None and fusion.filter:
            xk, Pk = np.array(fusion.model.x0, np.float64), np.array(fusion.model.P0, np.float64)
        for k, st in enumerate(steps):
            n = int(st["n"][s])
            tag = f"{fusion_name} stream {s} step {k}"
            rec, erec, rows = st["rec"][s], st["epi"][0][s], st["epi"][1][s]
            use_imu = fusion is not None and fusion.use_imu
            nrm, om = (st["imu"][s, 15:18], st["imu"][s, 18:21]) if use_imu else (None, sensors[s, 4:7])
            R = st["imu"][s, 6:15].reshape(3, 3) if use_imu else sensors[s, 7:16].reshape(3, 3)
            before = rec.copy(); before[0:4] = erec[6:10]
            keepf = st["keep"][s, :n].astype(bool) if fusion is not None else None
            ref = er.pair_epi(st["old"][s, :n], st["nxt"][s, :n], st["keep"][s, :n], sensors[s], before, anchor_px=EPI["anchor"],
                              anchor_min=EPI["anchor_min"], sigma_max=EPI["sigma_max"], keep=keepf, nrm=nrm, omega=om if use_imu else None,
                              solved=fusion is None or rec[15] != 0)
            assert ref["flag"] == 0, (tag, ref["flag"])
            assert_epi_close(rec[0:3], rec[3], erec, rows[:n], ref, tag)
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
                assert np.array_equal(st["imu_after"][s, 0:3], rec[8:11]), tag         # the epipolar v_uav, not the solve's
    print(f"{fusion_name}: largest deviation of (t^, s) so far {SEEN['dev']:.3e}")


def test_stream_refusals(pkg, ofk):
    from of_amd.pipeline import FlowStream, PipelineConfig, FusionConfig
    fs = FlowStream(W, H, batch=1, cfg=PipelineConfig.of_module(), fusion=FusionConfig.of_module())
    try:
        fs.ctx.set_epipolar(**EPI)
        prev, nxt, _ = pair_frames(1)
        fs.begin(prev)
        with pytest.raises(ofk.OfkError, match="sensor model"):
            fs.step_fused(nxt, ofk.make_sensors(1))
    finally:
        fs.close()
    cfg = PipelineConfig(max_corners=CORNERS, quality=0.01, min_distance=6, block_size=5, win=15, max_level=2, max_count=20, eps=0.03)
    for name, kw in (("ofk_set_cov", dict(set_cov=dict(mode="propagate", sigma_flow=0.3))), ("ofk_set_joint", dict(set_joint=dict(sigma_flow=0.2))),
                     ("ofk_set_plane", dict(set_plane=dict(sigma_flow=0.2)))):
        fs = FlowStream(W, H, batch=1, cfg=cfg, fusion=FusionConfig.node())
        try:
            fs.ctx.set_epipolar(**EPI)
            for fn, args in kw.items():
                getattr(fs.ctx, fn)(**args)
            prev, nxt, _ = pair_frames(1)
            fs.begin(prev)
            with pytest.raises(ofk.OfkError, match=name):
                fs.step_fused(nxt, ofk.make_sensors(1))
        finally:
            fs.close()
