"""The finite motion on the device (include/ofk.h: ofk_set_finite_motion) against tests/finite_reference.py.

Stage entry: within one float32 ulp of the restatement (sin and cos come from two math libraries), bit for bit (compared as uint32)
where omega = 0, the path without them; slots beyond counts keep a sentinel; every fallback condition; out == in.  Where a result is
not a number only that is compared: IEEE 754 leaves the sign and payload of a NaN an operation creates to the implementation.
Resident chains: every check is a composition of stage entries - the points the solve saw are ofk_finite_correct_points of the
rolling shutter's points of the camera's points of the downloaded raw points, the records are the reference solve of those points,
and everything that lives in the image is bit-identical to a run with the setting off.  The stream steps are also held, step by step,
to stream_oracle.NodeLoop with the solver fed from the rewritten points (finite_reference.finite_loop).  Frame sizes, slice counts
and overlap settings are tests/test_gpu_rs.py's: both take their scene from tests/rs_scene.py.

The rendered scene (480 x 640, motion="finite", row 2's motion, LK on 4 levels, seeded from the sensor model), measured on an MI355X:
190 tracked points, largest tracked flow 35.4 px, |v - T| / |T| 0.03330 with the setting off and 0.00422 with it on.  (Unseeded, LK
loses most of the points at this flow: 0.57680 off, 0.41016 on - the tracker's error, which is why finite_reference.scene seeds.)"""
import numpy as np
import pytest

import batch_oracle as BO
import cov_reference as cr
import finite_reference as F
import joint_reference as J
import plane_reference as P
import rs_reference as R
import rs_scene as TR
from joint_checks import JOINT, assert_joint_close
from plane_checks import PLANE, assert_plane_close
from point_stage_helpers import ROBUST, SENTINEL, assert_image_side_identical, assert_plain_records, bits, robust_reference, same_points
from stream_oracle import feasibility_solve, imu_messages, plain_solve

pytestmark = pytest.mark.gpu

H, W, B = TR.H, TR.W, TR.B
FM = F.setting(F.EXACT, 0.1)


def as_struct(ofk, fm):
    return ofk.FiniteMotion(fm["mode"], fm["min_depth"])


@pytest.fixture(scope="module")
def sctx(ofk):
    c = ofk.Context(0, 64, 48, 3, 300, 2)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------- the stage entry
FALLBACKS = 8


def stage_points(seed):
    """(prev, next [3,300,2] f32, sensors [3,28]) over a 1280 x 960 frame and a border around it; image 1 has omega = 0 (theta^2 <
    1e-16: no transcendentals), and the first points of image 2 are placed to hit every fallback condition but scaling == 0 (a whole
    image's) and the depth (image 1 turned by 1.5 rad: both in the test)."""
    rng = np.random.default_rng(seed)
    p0 = np.stack([rng.uniform(-60, 1340, (3, 300)), rng.uniform(-50, 1010, (3, 300))], -1)
    p1 = p0 + np.stack([rng.uniform(-60, 60, (3, 300)), rng.uniform(-70, 70, (3, 300))], -1)
    p0, p1 = p0.astype(np.float32), p1.astype(np.float32)
    sn = np.zeros((3, 28))
    nrm = (F.tilted_normal(3.0), F.tilted_normal(10.0), np.array([1.0, 0.0, 0.0]))          # image 2: the plane's horizon is the column x = cx
    for b, om in enumerate(((0.02, -0.03, 0.15), (0.0, 0.0, 0.0), (-0.004, 0.003, -0.05))):
        sn[b, 0] = 1.0 + 0.1 * b; sn[b, 1:4] = nrm[b]; sn[b, 4:7] = om; sn[b, 7:16] = np.eye(3).ravel()
        sn[b, 19:22] = (1e-3, 1.25e-3, 9e-4)[b], (640.0, 652.3, 600.0)[b], (480.0, 470.1, 500.0)[b]
    p0[2, :, 0] = np.abs(p0[2, :, 0] - 600.0) + 640.0; p1[2, :, 0] = np.abs(p1[2, :, 0] - 600.0) + 640.0      # image 2: both ends right of the horizon
    p1[2, 0] = (600.0, 400.0)                                    # den = n.p1 = 0
    p0[2, 1] = (300.0, 500.0)                                    # n.q~ < 0 < n.p1: s < 0
    p1[2, 2] = (np.nan, 480.0); p1[2, 3] = (900.0, np.nan); p0[2, 4] = (np.nan, 300.0); p1[2, 5] = (np.inf, 300.0)
    p0[2, 6] = (3e9, 500.0)                                      # a result beyond 1e6
    p1[2, 7] = (600.0 + 1e-11, 400.0)                            # |den| < 1e-12 would need more than f32 holds next to 600: den = 0 again
    return p0, p1, sn


def test_stage_entry_against_the_restatement(ofk, sctx):
    p0, p1, sn = stage_points(31)
    m = as_struct(ofk, FM)
    for counts in ((0, 257, 300), (1, 255, 256), (300, 300, 8)):
        a, b = sctx.finite_correct_points(m, p0, p1, counts, sensors=sn, out=(np.full(p0.shape, SENTINEL), np.full(p0.shape, SENTINEL)))
        ra, rb, good = F.correct_points(FM, p0, p1, sn, full=True)
        for i, n in enumerate(counts):
            ulp = 0 if i == 1 else 1                             # image 1: omega = 0
            assert same_points(a[i, :n], ra[i, :n], ulp) and same_points(b[i, :n], rb[i, :n], ulp), (counts, i)
            assert np.all(a[i, n:] == SENTINEL) and np.all(b[i, n:] == SENTINEL), (counts, i)
    assert not good[2, :FALLBACKS].any() and good[2, FALLBACKS:].all() and good[0].all() and good[1].all()
    assert np.array_equal(bits(a[2, :FALLBACKS]), bits(p0[2, :FALLBACKS])) and np.array_equal(bits(b[2, :FALLBACKS]), bits(p1[2, :FALLBACKS]))
    assert np.abs(b[0] - p1[0]).max() > 1.0 and np.abs(b[1] - p1[1]).max() > 1.0            # the rewrite is not the identity
    # scaling == 0: the fallback for the whole of image 0; the depth: image 1 turned by 1.5 rad about y, and the setting's threshold
    s0 = sn.copy(); s0[0, 19] = 0.0; s0[1, 4:7] = (0.0, 1.5, 0.0)
    for fm in (FM, F.setting(F.EXACT, 0.01), F.setting(F.EXACT, 1.0)):
        a, b = sctx.finite_correct_points(as_struct(ofk, fm), p0, p1, sensors=s0)
        ra, rb, good = F.correct_points(fm, p0, p1, s0, full=True)
        assert not good[0].any() and np.array_equal(bits(a[0]), bits(p0[0])) and np.array_equal(bits(b[0]), bits(p1[0]))
        assert same_points(a, ra, 1) and same_points(b, rb, 1)
    depth = [F.correct_points(F.setting(F.EXACT, t), p0, p1, s0, full=True)[2][1].sum() for t in (0.01, 0.1, 1.0)]
    assert depth[0] > depth[1] > depth[2] == 0, depth            # the threshold decides, and the three settings differ on these points


def test_stage_entry_small_batches_aliasing_and_batch_3(ofk, sctx):
    p0, p1, sn = stage_points(77)
    m = as_struct(ofk, FM)
    a, b = sctx.finite_correct_points(m, p0[:1, :1], p1[:1, :1], sensors=sn[:1])
    ra, rb = F.correct_points(FM, p0[:1, :1], p1[:1, :1], sn[:1])
    assert a.shape == (1, 1, 2) and same_points(a, ra, 1) and same_points(b, rb, 1) and not np.array_equal(b, p1[:1, :1])
    a, b = sctx.finite_correct_points(m, p0[0, :3], p1[0, :3], sensors=sn[:1])
    assert a.shape == (3, 2) and same_points(b, F.correct_points(FM, p0[0, :3], p1[0, :3], sn[:1])[1], 1)
    # out == in on the host side only: the entry uploads into four distinct device buffers whatever the caller aliases, so the kernel's
    # in-place path (in == out on the device) is not run here; the resident chains with the camera or the rolling shutter on run it
    # (test_each_setting_with_the_finite_motion_on[camera / rs / several])
    counts = (17, 300, 123)
    a, b = sctx.finite_correct_points(m, p0, p1, counts, sensors=sn, out=(p0, p1))
    ra, rb = F.correct_points(FM, p0, p1, sn)
    for i, n in enumerate(counts):
        assert same_points(a[i, :n], ra[i, :n], 1) and same_points(b[i, :n], rb[i, :n], 1), i
        assert np.array_equal(bits(a[i, n:]), bits(p0[i, n:])) and np.array_equal(bits(b[i, n:]), bits(p1[i, n:])), i
    lib = ofk.load_library()                                     # and the same host arrays as input and output of the C entry
    q0, q1 = p0.copy(), p1.copy()
    c = np.asarray(counts, np.int32)
    assert lib.ofk_finite_correct_points(sctx._h, ofk.C.byref(m), q0.ctypes.data, q1.ctypes.data, c.ctypes.data, 3, 300, sn.ctypes.data, q0.ctypes.data,
                                         q1.ctypes.data) == 0
    assert np.array_equal(bits(q0), bits(a)) and np.array_equal(bits(q1), bits(b))


def test_finite_points_helper(pkg, ofk):
    """velocity_node.finite_points on one image's [N,2] points with a [28] row and on a batch, against the restatement."""
    from of_amd.velocity_node import finite_points
    p0, p1, sn = stage_points(5)
    a, b = finite_points(p0[0], p1[0], sn[0])
    ra, rb = F.correct_points(FM, p0[0], p1[0], sn[0])
    assert a.shape == (300, 2) and a.dtype == np.float32 and same_points(a, ra, 1) and same_points(b, rb, 1) and not np.array_equal(b, p1[0])
    a, b = finite_points(p0, p1, sn, min_depth=0.5)
    ra, rb = F.correct_points(F.setting(F.EXACT, 0.5), p0, p1, sn)
    assert a.shape == (3, 300, 2) and same_points(a, ra, 1) and same_points(b, rb, 1)


# ---------------------------------------------------------------------------------------------------- frame pairs
def rewritten_of_download(ctx, ofk, out, sensors, tag, camera=None, rs=None):
    """ofk_finite_download == ofk_finite_correct_points of (ofk_rs_correct_points of (ofk_undistort_points of)) the downloaded raw
    points - one kernel, twice: bit for bit - and within one ulp per stage of the numpy restatements of the same chain."""
    nb = len(out["counts"])
    pu, nu = ctx.finite_download(nb)
    q0, q1 = out["prev_pts"], out["next_pts"]
    r0, r1 = q0, q1
    if camera is not None:
        q0, q1 = ctx.undistort_points(camera, q0, out["counts"]), ctx.undistort_points(camera, q1, out["counts"])
        r0, r1 = q0, q1                                          # the camera's restatement is test_gpu_camera's business
    if rs is not None:
        kw = dict(ideal_prev=q0, ideal_next=q1) if camera is not None else {}
        q0, q1 = ctx.rs_correct_points(TR.as_struct(ofk, rs), out["prev_pts"], out["next_pts"], out["counts"], sensors=sensors, **kw)
        r0, r1 = q0, q1                                          # the rolling shutter's is test_gpu_rs's
    sp, sn = ctx.finite_correct_points(as_struct(ofk, FM), q0, q1, out["counts"], sensors=sensors)
    rp, rn = F.correct_points(FM, r0, r1, sensors)
    moved = 0.0
    for b in range(nb):
        n = int(out["counts"][b])
        assert n > 8, (tag, b, n)
        assert np.array_equal(bits(pu[b, :n]), bits(sp[b, :n])) and np.array_equal(bits(nu[b, :n]), bits(sn[b, :n])), (tag, b)
        assert same_points(pu[b, :n], rp[b, :n], 1) and same_points(nu[b, :n], rn[b, :n], 1), (tag, b)
        ok = out["status"][b, :n] == 1
        moved = max(moved, float(np.abs(nu[b, :n][ok] - q1[b, :n][ok]).max()))
    assert moved > 0.01, (tag, moved)                            # the rewrite is not the identity on this scene
    return pu, nu


@pytest.mark.parametrize("streams,overlap", [(1, False), (1, True), (2, False), (2, True)])
def test_pairs_run_is_a_composition_of_stage_entries(pkg, ofk, streams, overlap):
    from of_amd.pipeline import FlowPipeline
    prev, nxt, sensors = TR.pair_batch(pkg, ofk)
    tag = (streams, overlap)
    pipe = FlowPipeline(W, H, B, TR.pair_cfg(), streams=streams)
    try:
        pipe.ctx.set_overlap(overlap)
        pipe.upload(prev, nxt, sensors)
        never = pipe.run()
        with pytest.raises(ofk.OfkError):
            pipe.ctx.finite_download(B)
        pipe.ctx.set_finite_motion(as_struct(ofk, FM))
        on = pipe.run()
        pu, nu = rewritten_of_download(pipe.ctx, ofk, on, sensors, tag)
        ip, inx = pipe.ideal_points()
        assert np.array_equal(bits(ip), bits(pu)) and np.array_equal(bits(inx), bits(nu))
        for other in (pipe.ctx.camera_download, pipe.ctx.rs_download):          # no run with either on: their downloads keep their contract
            with pytest.raises(ofk.OfkError):
                other(B)
        again = pipe.run()                                       # the slices free-run over consecutive calls
        pipe.ctx.set_finite_motion(None)
        off = pipe.run()
    finally:
        pipe.close()
    assert_image_side_identical(on, never, tag)
    assert_plain_records(on, pu, nu, sensors, tag)
    assert np.abs(on["records"][:, :3] - never["records"][:, :3]).max() > 1e-6           # the rewrite reached the solve
    BO.assert_records_identical(again["records"], on["records"], tag)
    assert_image_side_identical(off, never, tag)
    BO.assert_records_identical(off["records"], never["records"], tag)


@pytest.mark.parametrize("setting", ["robust", "cov", "gate", "seed", "camera", "rs", "joint", "plane", "several"])
def test_each_setting_with_the_finite_motion_on(pkg, ofk, setting):
    """Pair runs on two slices; `several` = camera, rolling shutter, gates, seed and covariance at once.  (The zones belong to the
    streams.)"""
    from of_amd.pipeline import CameraModel, FlowPipeline
    prev, nxt, sensors = TR.pair_batch(pkg, ofk)
    cfg = {"robust": {}, "cov": TR.COV, "gate": TR.GATE, "seed": TR.SEED, "camera": {}, "rs": {}, "joint": {}, "plane": {},
           "several": dict(TR.COV, **TR.GATE, **TR.SEED)}[setting]
    cam = CameraModel(**TR.PAIR_CAM).setting() if setting in ("camera", "several") else None
    rs = R.rshutter(R.GYRO, -0.9, 0.0, H, omega_gain=1.0) if setting in ("rs", "several") else None
    pipe = FlowPipeline(W, H, B, TR.pair_cfg(**cfg), streams=2)
    try:
        if setting == "robust":
            pipe.ctx.set_robust(**ROBUST)
        if cam is not None:
            pipe.ctx.set_camera(cam)
        if rs is not None:
            pipe.ctx.set_rolling_shutter(TR.as_struct(ofk, dict(rs, rows=0)))
        if setting == "joint":
            pipe.ctx.set_joint(**JOINT)
        if setting == "plane":
            pipe.ctx.set_plane(**PLANE)
        pipe.upload(prev, nxt, sensors)
        off = pipe.run()
        pipe.ctx.set_finite_motion(as_struct(ofk, FM))
        on = pipe.run()
        pu, nu = rewritten_of_download(pipe.ctx, ofk, on, sensors, setting, camera=cam, rs=rs)
        if cam is not None:                                      # every download is "what the solve stage saw"
            cp, cn = pipe.ctx.camera_download(B)
            assert np.array_equal(bits(cp), bits(pu)) and np.array_equal(bits(cn), bits(nu))
        if rs is not None:
            cp, cn = pipe.ctx.rs_download(B)
            assert np.array_equal(bits(cp), bits(pu)) and np.array_equal(bits(cn), bits(nu))
        if setting == "robust":
            wts, st = pipe.ctx.robust_download(B)
        if setting in ("cov", "several"):
            cov = pipe.covariances()
        if setting in ("gate", "several"):
            stats = pipe.track_gate_stats()
        if setting == "joint":                                   # the solve's own record of the rewritten points: what the joint kernel started from
            jrec = pipe.ctx.joint_download(B)
            pipe.ctx.set_joint(None)
            before = pipe.run()
        if setting == "plane":
            prec = pipe.ctx.plane_download(B)
            pipe.ctx.set_plane(None)
            before = pipe.run()
    finally:
        pipe.close()
    assert_image_side_identical(on, off, setting)             # a seeded LK predicts its seeds exactly as with the setting off
    assert np.abs(on["records"][:, :3] - off["records"][:, :3]).max() > 1e-6
    if setting not in ("robust", "joint", "plane"):
        assert_plain_records(on, pu, nu, sensors, setting)
    if setting in ("gate", "several"):
        assert stats[:, 0].min() > 8, stats
    for b in range(B):
        n = int(on["counts"][b]); sr = sensors[b]
        ok = on["status"][b, :n] == 1
        new = nu[b, :n].astype(np.float64); old = pu[b, :n].astype(np.float64)
        x = (new - [sr[20], sr[21]]) * sr[19]; u = (new - old) * sr[19]
        if setting == "robust":
            ref = robust_reference(b, x, u, ok, sr, st[b])
            np.testing.assert_allclose(on["records"][b, 0:3], ref["v"], rtol=0, atol=1e-10, err_msg=str(b))
            np.testing.assert_allclose(wts[b, :n], ref["weights"], rtol=0, atol=1e-9, err_msg=str(b))
        if setting in ("cov", "several"):
            ref = cr.pair_record(cr.NODE, pu[b, :n], nu[b, :n], on["status"][b, :n], sr, TR.COVD, on["records"][b])
            assert ref[13] == 0 and cov[b, 13] == 0
            for sl in (slice(0, 6), slice(6, 12), slice(16, 22)):
                assert np.abs(cov[b, sl] - ref[sl]).max() <= 1e-9 * np.abs(ref[sl]).max(), (b, sl)
        if setting == "joint":                                   # the joint solve of the rewritten points: its own reference and tolerances
            ref = J.pair_joint(J.NODE, pu[b, :n], nu[b, :n], on["status"][b, :n], sr, JOINT["sigma_flow"], (JOINT["sigma_omega"],) * 3,
                               before["records"][b])
            assert_joint_close(on["records"][b, 0:3], on["records"][b, 3], jrec[b], ref, f"finite motion, pair {b}")
        if setting == "plane":
            ref = P.pair_plane(P.NODE, pu[b, :n], nu[b, :n], on["status"][b, :n], sr, PLANE["sigma_flow"], PLANE["sigma_normal"],
                               before["records"][b])
            assert_plane_close(on["records"][b, 0:3], on["records"][b, 3], prec[b], ref, f"finite motion, pair {b}")


# ---------------------------------------------------------------------------------------------------- streams
SH, SW, NB, NSTEPS, MIN_FEAT, RADIUS, FEAS_T = TR.SH, TR.SW, TR.NB, TR.NSTEPS, TR.MIN_FEAT, TR.RADIUS, TR.FEAS_T


def run_stream(ofk, kind, frames, sensors, cfg, fm):
    """The device's steps: per step dict(rec, tracks, counts, nxt, keep, zones, ideal)."""
    from of_amd.pipeline import FlowStream, FusionConfig
    fusion = None if kind == "step" else FusionConfig(use_imu=False, redetect_replace=kind == "replace")
    fs = FlowStream(SW, SH, batch=NB, cfg=cfg, min_features=MIN_FEAT, mask_radius=RADIUS, fusion=fusion)
    try:
        if fm is not None:
            fs.ctx.set_finite_motion(fm)
        tracks, counts = fs.begin(frames[:, 0])
        steps = [dict(tracks=tracks, counts=counts)]
        for t in range(1, frames.shape[1]):
            out = fs.step(frames[:, t], sensors) if kind == "step" else fs.step_fused(frames[:, t], sensors)
            nxt, keep = fs.ctx.stream_last_points(cfg.max_corners)
            steps.append(dict(rec=out[0], tracks=out[-2], counts=out[-1], nxt=nxt, keep=keep, zones=fs.zones(),
                              ideal=fs.ideal_points() if fm is not None else None))
        return steps
    finally:
        fs.close()


@pytest.mark.parametrize("kind", ["step", "fused", "replace"])
def test_stream_steps_with_zones_and_the_finite_motion(pkg, ofk, sctx, kind):
    frames, sensors, cfg = TR.stream_setup(pkg, ofk, kind)
    m = as_struct(ofk, FM)
    on = run_stream(ofk, kind, frames, sensors, cfg, m)
    off = run_stream(ofk, kind, frames, sensors, cfg, None)
    given = [dict() for _ in range(NB)]
    loops = [F.finite_loop(frames[b, 0], cfg, MIN_FEAT, RADIUS, FM, sensors[b], plain_solve if kind == "step" else feasibility_solve(sensors[b, 22:25], FEAS_T, 2),
                           given=given[b], zones={}, replace=kind == "replace") for b in range(NB)]
    for b in range(NB):
        assert np.array_equal(bits(on[0]["tracks"][b, :on[0]["counts"][b]]), bits(loops[b].tracks))
    same, solved, moved = True, 0, 0.0                           # the image side equals the setting-off run's until the keep flags part
    for t in range(1, NSTEPS + 1):
        s, s_off = on[t], off[t]
        for b in range(NB):
            tag = (kind, t, b)
            given[b]["pts"] = (s["ideal"][0][b], s["ideal"][1][b])     # the solver takes the device's rewritten points: one ulp apart
            o = loops[b].step(frames[b, t], sensors[b])
            n = o["n_old"]
            assert n > 0, tag
            assert np.array_equal(bits(s["nxt"][b, :n]), bits(o["new"])), tag
            pu, nu = s["ideal"][0][b, :n], s["ideal"][1][b, :n]
            sp, sn = sctx.finite_correct_points(m, o["old"], s["nxt"][b, :n], sensors=sensors[b:b + 1])
            assert np.array_equal(bits(pu), bits(sp)) and np.array_equal(bits(nu), bits(sn)), tag          # the composition
            assert same_points(pu, o["ideal"][0], 1) and same_points(nu, o["ideal"][1], 1), tag
            if o["keep"].any():
                moved = max(moved, float(np.abs(nu - s["nxt"][b, :n])[o["keep"]].max()))
            rec = s["rec"][b]
            assert rec[12] == n and rec[13] == o["n_tracked"] and rec[11] == o.get("used", o["n_tracked"]) and s["counts"][b] == len(o["tracks"]), (tag, rec[11:14])
            assert np.array_equal(s["keep"][b, :n] != 0, o["keep"]), tag
            assert np.array_equal(bits(s["tracks"][b, :s["counts"][b]]), bits(o["tracks"].astype(np.float32))), tag
            if o["solved"]:
                solved += 1
                np.testing.assert_allclose(rec[:3], o["v"], rtol=0, atol=1e-10, err_msg=str(tag))
                np.testing.assert_allclose(rec[8:11], o["v_uav"], rtol=0, atol=1e-10, err_msg=str(tag))
        if same:
            assert np.array_equal(bits(s["nxt"]), bits(s_off["nxt"])), (kind, t)            # same tracks in, same LK out
            same = np.array_equal(s["keep"], s_off["keep"])
            if same:
                assert np.array_equal(s["counts"], s_off["counts"]) and np.array_equal(bits(s["tracks"]), bits(s_off["tracks"])), (kind, t)
                for k in ("zones", "motion", "stats"):
                    assert np.array_equal(bits(s["zones"][k]), bits(s_off["zones"][k])), (kind, t, k)
                assert np.abs(s["rec"][:, :3] - s_off["rec"][:, :3]).max() > 1e-8        # and yet another solve
    print(f"{kind}: solved {solved}, largest rewrite {moved:.3f} px, image side equal to the setting off throughout: {same}")
    redetected = sum(1 for t in range(1, NSTEPS + 1) if (on[t - 1]["counts"] <= MIN_FEAT).any())
    assert solved >= NB * NSTEPS - 2 and moved > 0.003 and redetected > 0


def test_fused_step_takes_normal_and_omega_from_the_imu_state(pkg, ofk, sctx):
    """Under ofk_fusion.use_imu the rewrite reads the resident IMU state's normal [15..17] and omega [18..20], as k_stream_fuse does."""
    from of_amd.pipeline import FlowStream, FusionConfig
    frames, sensors, cfg = TR.stream_setup(pkg, ofk, "fused")
    m = as_struct(ofk, FM)
    rng = np.random.default_rng(8)
    fs = FlowStream(SW, SH, batch=NB, cfg=cfg, min_features=MIN_FEAT, mask_radius=RADIUS, fusion=FusionConfig.node())
    try:
        fs.ctx.set_finite_motion(m)
        tracks, counts = fs.begin(frames[:, 0])
        fs.push_imu(np.stack([imu_messages(rng, 50.0 + 3 * b, 3, tilt=0.05, rate=(0.01, -0.02, 0.04), rate_sigma=0.001) for b in range(NB)]))
        st, _ = fs.ctx.imu_state(NB)
        fs.step_fused(frames[:, 1], sensors)
        nxt, _ = fs.ctx.stream_last_points(cfg.max_corners)
        pu, nu = fs.ideal_points()
    finally:
        fs.close()
    src = sensors.copy()
    src[:, 1:4] = st[:, 15:18]; src[:, 4:7] = st[:, 18:21]
    assert np.abs(src[:, 4:7] - sensors[:, 4:7]).max() > 1e-3 and np.abs(src[:, 1:4] - sensors[:, 1:4]).max() > 1e-3
    old = tracks[:, :cfg.max_corners]
    sp, sn = sctx.finite_correct_points(m, old, nxt, counts, sensors=src)
    rp, rn = F.correct_points(FM, old, nxt, sensors, normal=st[:, 15:18], omega=st[:, 18:21])
    wp, wn = F.correct_points(FM, old, nxt, sensors)             # what the sensors' own normal and omega would have given
    for b in range(NB):
        n = int(counts[b])
        assert n > 8
        assert np.array_equal(bits(pu[b, :n]), bits(sp[b, :n])) and np.array_equal(bits(nu[b, :n]), bits(sn[b, :n])), b
        assert same_points(pu[b, :n], rp[b, :n], 1) and same_points(nu[b, :n], rn[b, :n], 1), b
        assert not same_points(nu[b, :n], wn[b, :n], 1), b


def test_off_is_off(pkg, ofk):
    """A context that ran streams with the setting on (its buffers exist) and had it switched off returns, from the next begin on, the
    bits of a context that never heard of the setting - for the plain and the fused step.  Records, tracks, points, keep flags and zones
    are compared, and a context with the setting off has nothing to download.  The launch count is NOT compared: the context keeps
    no count of kernel launches (its stage timers bracket stages, and the rewrite sits inside the tracker's bracket), so a launch with
    the setting off that wrote nothing would pass here.  The call site in track() is the one guard (DESIGN.md says so)."""
    from of_amd.pipeline import FlowStream, FusionConfig
    for fused in (False, True):
        frames, sensors, cfg = TR.stream_setup(pkg, ofk, "fused" if fused else "step")
        res = []
        for touch in (False, True):
            fs = FlowStream(SW, SH, batch=NB, cfg=cfg, min_features=MIN_FEAT, mask_radius=RADIUS, fusion=FusionConfig(use_imu=False) if fused else None)
            step = (lambda t: fs.step_fused(frames[:, t], sensors)) if fused else (lambda t: fs.step(frames[:, t], sensors))
            try:
                if touch:
                    fs.ctx.set_finite_motion(mode="exact")
                    fs.begin(frames[:, 0])
                    step(1); step(2)
                    fs.ideal_points()
                    fs.ctx.set_finite_motion(None)
                    assert fs.ctx.get_finite_motion().mode == ofk.FM_OFF
                    fs.ctx.zones_reset()
                else:
                    with pytest.raises(ofk.OfkError):
                        fs.ctx.finite_download(NB)
                fs.begin(frames[:, 0])
                res.append([tuple(step(t)) + tuple(fs.ctx.stream_last_points(cfg.max_corners)) + (fs.zones(),) for t in range(1, NSTEPS + 1)])
                if not touch:
                    with pytest.raises(ofk.OfkError):            # still nothing: no buffer was allocated, no rewrite ran
                        fs.ctx.finite_download(NB)
            finally:
                fs.close()
        for t, (x, y) in enumerate(zip(*res)):
            for i in range(len(x) - 1):
                assert np.array_equal(bits(x[i]), bits(y[i])), (fused, t, i)
            for k in ("zones", "motion", "stats"):
                assert np.array_equal(bits(x[-1][k]), bits(y[-1][k])), (fused, t, k)


# ---------------------------------------------------------------------------------------------------- refusals
def test_the_three_refusals_by_run_and_step(pkg, ofk):
    """OFK_SOLVE_OFMODULE, OFK_FLOW_ROTATIONAL and OFK_KEEP_LEGACY are not the sensor model: with the setting on the fused step refuses
    each before any launch (the pair run and the plain step take NODE and SIM alone, setting or not), the setting stays, and the same
    step passes with the setting off."""
    from of_amd.pipeline import FlowPipeline, FlowStream, FusionConfig
    frames, sensors, cfg = TR.stream_setup(pkg, ofk, "fused")
    m = as_struct(ofk, FM)
    for name, fu, variant in (("ofmodule", dict(keep=ofk.KEEP_LEGACY), ofk.SOLVE_OFMODULE), ("rotational", dict(flow=ofk.FLOW_ROTATIONAL), ofk.SOLVE_NODE),
                              ("legacy", dict(keep=ofk.KEEP_LEGACY), ofk.SOLVE_NODE)):
        c = type(cfg)(**{**cfg.__dict__, "solve_variant": variant, "zones": "off"})
        fs = FlowStream(SW, SH, batch=NB, cfg=c, min_features=MIN_FEAT, mask_radius=RADIUS, fusion=FusionConfig(use_imu=False, **fu))
        try:
            fs.ctx.set_finite_motion(m)
            fs.begin(frames[:, 0])
            with pytest.raises(ofk.OfkError) as e:
                fs.step_fused(frames[:, 1], sensors)
            assert e.value.code == ofk.E_INVALID and "finite" in str(e.value), (name, str(e.value))
            assert fs.ctx.get_finite_motion().mode == ofk.FM_EXACT
            with pytest.raises(ofk.OfkError):                    # refused before anything ran: nothing to download
                fs.ctx.finite_download(NB)
            fs.ctx.set_finite_motion(None)
            fs.step_fused(frames[:, 1], sensors)
        finally:
            fs.close()
    prev, nxt, psn = TR.pair_batch(pkg, ofk)
    pipe = FlowPipeline(W, H, B, TR.pair_cfg(solve_variant=ofk.SOLVE_OFMODULE))
    try:
        pipe.ctx.set_finite_motion(m)
        pipe.upload(prev, nxt, psn)
        with pytest.raises(ofk.OfkError) as e:
            pipe.run()
        assert e.value.code == ofk.E_INVALID
        with pytest.raises(ofk.OfkError):
            pipe.ctx.finite_download(B)
    finally:
        pipe.close()
    fs = FlowStream(SW, SH, batch=NB, cfg=type(cfg)(**{**cfg.__dict__, "solve_variant": ofk.SOLVE_OFMODULE}), min_features=MIN_FEAT, mask_radius=RADIUS)
    try:
        fs.ctx.set_finite_motion(m)
        fs.begin(frames[:, 0])
        with pytest.raises(ofk.OfkError) as e:
            fs.step(frames[:, 1], sensors)
        assert e.value.code == ofk.E_INVALID
    finally:
        fs.close()


# ---------------------------------------------------------------------------------------------------- the rendered scene
def test_rendered_scene_with_finite_motion_on_the_device(pkg, ofk):
    """One pair rendered as the exact rigid motion at row 2's motion, through the device chain: the error with the setting on is below
    the error with it off.  No threshold beyond the inequality: LK's own error at 42 px of flow is what is left."""
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    fr, sr, cfg = F.scene()
    s = F.SCENE
    pipe = FlowPipeline(s["w"], s["h"], 1, cfg)
    try:
        pipe.upload(fr["prev"][None], fr["next"][None], sr[None])
        off = pipe.run()
        pipe.ctx.set_finite_motion(as_struct(ofk, FM))
        on = pipe.run()
        pu, nu = pipe.ideal_points()
    finally:
        pipe.close()
    n = int(on["counts"][0])
    ok = on["status"][0, :n] == 1
    assert ok.sum() > 50
    assert_image_side_identical(on, off, "scene")
    ra, rb = F.correct_points(FM, on["prev_pts"][0, :n], on["next_pts"][0, :n], sr[None])
    assert same_points(pu[0, :n], ra, 1) and same_points(nu[0, :n], rb, 1)
    np.testing.assert_allclose(on["records"][0, :3], F.solve_points(pu[0, :n][ok], nu[0, :n][ok], sr), rtol=0, atol=1e-10)
    e_on, e_off = F.error(on["records"][0, :3], s["T"]), F.error(off["records"][0, :3], s["T"])
    flow = float(np.sqrt(((on["next_pts"][0, :n][ok] - on["prev_pts"][0, :n][ok]) ** 2).sum(-1)).max())
    print(f"rendered scene: {int(ok.sum())} points, largest flow {flow:.1f} px, |v - T| / |T| off {e_off:.5f} on {e_on:.5f}")
    assert e_on < e_off, (e_on, e_off)
