"""The camera model on the device (include/ofk.h: ofk_set_camera) against tests/camera_reference.py.

Stage entries: Brown bit for bit (compared as uint32), the fisheye within one float32 ulp (tan and atan come from two math
libraries); slots beyond counts keep a sentinel; the fallback rule.  Where a result is not a number only that is compared: IEEE 754
leaves the sign and payload of a NaN an operation creates to the implementation.
Resident chains: every check is a composition of stage entries - the ideal points the solve saw are ofk_undistort_points of the
downloaded raw points, the records are the reference solve of those ideal points, and everything that lives in the image is
bit-identical to a run with the camera off.  The stream steps are also held, step by step, to stream_oracle.NodeLoop with the solver
fed from the ideal points (camera_reference.camera_loop).

The distorted 480 x 640 scene of tests/test_camera_reference.py on the device gives that module's three figures (bit parity)."""
import numpy as np
import pytest

import batch_oracle as BO
import camera_reference as R
import combined_cases as cc
import cov_reference as cr
from point_stage_helpers import ROBUST, SENTINEL, assert_image_side_identical, assert_plain_records, bits, robust_reference, same_points
from stream_oracle import feasibility_solve

pytestmark = pytest.mark.gpu

H, W, B, CORNERS = 240, 320, 4, 64
MOTION = dict(v=(0.004, -0.003, 0.002), omega=(0.003, -0.002, 0.004), d=1.0)
PAIR_CAM = dict(fx=320.0, fy=320.0, cx=160.0, cy=120.0, k=R.STRONG[1])
_cache = {}


def as_struct(ofk, cam):
    """camera_reference's dict -> ofk.Camera, field by field (no defaults in between)."""
    import ctypes as C
    return ofk.Camera(cam["model"], cam["iters"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], (C.c_double * 8)(*cam["k"]), cam["fo_x"], cam["fo_y"],
                      cam["co_x"], cam["co_y"])


@pytest.fixture(scope="module")
def sctx(ofk):
    c = ofk.Context(0, 64, 48, 3, 300, 2)
    yield c
    c.close()


COUNTS = [(0, 1, 255), (256, 257, 300), (300, 17, 256), (1, 0, 299)]
BROWN = {
    "radial": dict(k=(-0.28, 0.09, 0.0, 0.0, -0.012)),
    "tangential": dict(k=R.STRONG[1]),
    "rational": dict(k=(-0.28, 0.09, 0.0, 0.0, -0.012, 0.02, -0.01, 0.003)),
    "rational-tangential-two-focals": dict(k=(0.11, -0.04, 0.0008, -0.0005, 0.006, 0.3, -0.02, 0.004), fo_x=870.0, fo_y=1130.0, co_x=600.5, co_y=500.25),
}


def frame_points(seed):
    """[3, 300, 2] f32 over the 1280 x 960 frame and a border of 60 pixels around it."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-60, 1340, (3, 300)), rng.uniform(-60, 1020, (3, 300))], -1).astype(np.float32)


def check_entries(ofk, ctx, cam, ulp, seed):
    m = as_struct(ofk, cam)
    pts = frame_points(seed)
    for counts in COUNTS:
        for fn, ref_fn in ((ctx.undistort_points, R.undistort_points), (ctx.distort_points, R.distort_points)):
            got = fn(m, pts, counts, out=np.full(pts.shape, SENTINEL))
            ref = ref_fn(cam, pts)
            for b, n in enumerate(counts):
                assert same_points(got[b, :n], ref[b, :n], ulp), (fn.__name__, counts, b)
                assert np.all(got[b, n:] == SENTINEL), (fn.__name__, counts, b)


@pytest.mark.parametrize("name", list(BROWN))
def test_brown_stage_entries_bit_for_bit(ofk, sctx, name):
    f = R.FRAME
    for iters in (1, 5, 20, 50):
        check_entries(ofk, sctx, R.camera(R.BROWN, BROWN[name]["k"], f["fx"], f["fy"], f["cx"], f["cy"], iters=iters,
                                          **{k: v for k, v in BROWN[name].items() if k != "k"}), 0, 20 + iters)


def test_fisheye_stage_entries_within_one_ulp(ofk, sctx):
    f = R.FRAME
    for iters in (1, 3, 10):
        check_entries(ofk, sctx, R.camera(R.FISHEYE, R.FISH[1], f["fx"], f["fy"], f["cx"], f["cy"], iters=iters), 1, 40 + iters)
    check_entries(ofk, sctx, R.camera(R.FISHEYE, (0.05, -0.01, 0.002, -0.0004), 400.0, 410.0, 640.0, 480.0, iters=10, fo_x=350.0, fo_y=360.0), 1, 44)
    # the centre itself: theta_d < 1e-8 takes s = 1
    cam = R.camera(R.FISHEYE, R.FISH[1], 1000.0, 1000.0, 652.0, 470.0)
    c = np.array([[[652.0, 470.0]]], np.float32)
    assert np.array_equal(sctx.undistort_points(as_struct(ofk, cam), c), c) and np.array_equal(sctx.distort_points(as_struct(ofk, cam), c), c)


def test_fallback_rule(ofk, sctx):
    nan, inf = np.nan, np.inf
    pts = np.array([[[100.0, 200.0], [nan, 5.0], [inf, 7.0], [3.0, -inf], [nan, nan], [1200.0, 900.0]]], np.float32)
    for cam in (R.frame_camera(R.STRONG, iters=20), R.frame_camera(R.FISH)):
        ulp = 0 if cam["model"] == R.BROWN else 1
        for fn, ref_fn in ((sctx.undistort_points, R.undistort_points), (sctx.distort_points, R.distort_points)):
            ref, good = ref_fn(cam, pts, full=True)
            assert good[0].tolist() == [True, False, False, False, False, True]
            assert same_points(fn(as_struct(ofk, cam), pts), ref, ulp), (cam["model"], fn.__name__)
    # coefficient sets that blow up at (500, 0) of a camera with f = 1000, c = 0 (tests/test_camera_reference.py): a pole and 2e10 pixels
    pts = np.array([[[500.0, 0.0], [100.0, 50.0]]], np.float32)
    for cam in (R.blow_up_camera(-4.0, 20), R.blow_up_camera(-3.9999999, 1)):
        ref, good = R.undistort_points(cam, pts, full=True)
        got = sctx.undistort_points(as_struct(ofk, cam), pts)
        assert good[0].tolist() == [False, True] and np.array_equal(bits(got), bits(ref)) and np.array_equal(got[0, 0], pts[0, 0])
    cam = R.camera(R.BROWN, (0, 0, 0, 0, 0, -4.0), 1000.0, 1000.0, 0.0, 0.0)
    got = sctx.distort_points(as_struct(ofk, cam), pts)
    assert np.array_equal(bits(got), bits(R.distort_points(cam, pts))) and np.array_equal(got[0, 0], pts[0, 0])


def test_cv2_facade(pkg, ofk):
    from of_amd import cv2_hip as cv2
    f = R.FRAME
    K = np.array([[f["fx"], 0, f["cx"]], [0, f["fy"], f["cy"]], [0, 0, 1.0]])
    src = frame_points(5)[0].reshape(-1, 1, 2)
    for D in (R.STRONG[1][:4], R.STRONG[1], BROWN["rational"]["k"]):
        got = cv2.undistortPoints(src, K, np.array(D))
        ref = R.undistort_points(R.camera(R.BROWN, D, f["fx"], f["fy"], f["cx"], f["cy"], iters=5, fo_x=1.0, fo_y=1.0, co_x=0.0, co_y=0.0), src)
        assert got.shape == src.shape and np.array_equal(bits(got), bits(ref))
    P = np.array([[900.0, 0, 640.0], [0, 910.0, 480.0], [0, 0, 1.0]])
    got = cv2.undistortPoints(src[:, 0], K, np.array(R.STRONG[1]), R=np.eye(3), P=P, criteria=(cv2.TERM_CRITERIA_COUNT | cv2.TERM_CRITERIA_EPS, 20, 1e-9))
    ref = R.undistort_points(R.camera(R.BROWN, R.STRONG[1], f["fx"], f["fy"], f["cx"], f["cy"], iters=20, fo_x=900.0, fo_y=910.0, co_x=640.0, co_y=480.0), src[:, 0])
    assert got.shape == (300, 2) and np.array_equal(bits(got), bits(ref))
    fish = R.camera(R.FISHEYE, R.FISH[1], f["fx"], f["fy"], f["cx"], f["cy"], iters=10, fo_x=1.0, fo_y=1.0, co_x=0.0, co_y=0.0)
    norm = cv2.fisheye.undistortPoints(src, K, np.array(R.FISH[1]))
    assert same_points(norm, R.undistort_points(fish, src), 1)
    back = cv2.fisheye.distortPoints(norm, K, np.array(R.FISH[1]))
    assert same_points(back, R.distort_points(fish, norm), 1) and np.abs(back - src).max() < 1e-3


# ---------------------------------------------------------------------------------------------------- frame pairs
def pair_batch(pkg, ofk):
    if "pairs" not in _cache:
        from of_amd import synth
        prev, nxt, base = synth.make_batch(B, H, W, seed=4300, distinct=B, margin=96, scaling=1.0 / PAIR_CAM["fx"], **MOTION)
        sensors = ofk.make_sensors(B, d=MOTION["d"], normal=base[0]["n"], omega=MOTION["omega"], offset=(0.02, -0.01, 0.2), scaling=1.0 / PAIR_CAM["fx"],
                                   cx=PAIR_CAM["cx"], cy=PAIR_CAM["cy"], v_prior=MOTION["v"])
        _cache["pairs"] = (prev, nxt, sensors)
    return _cache["pairs"]


def pair_cfg(**kw):
    from of_amd.pipeline import PipelineConfig
    return PipelineConfig(max_corners=CORNERS, quality=0.01, min_distance=8, block_size=7, win=15, max_level=3, max_count=20, eps=0.03, **kw)


def pair_camera(ofk):
    from of_amd.pipeline import CameraModel
    cm = CameraModel(**PAIR_CAM)
    return cm, R.camera(R.BROWN, PAIR_CAM["k"], PAIR_CAM["fx"], PAIR_CAM["fy"], PAIR_CAM["cx"], PAIR_CAM["cy"])


def ideal_of_download(ctx, m, cam, out, tag):
    """ofk_camera_download == ofk_undistort_points of the downloaded raw points == the numpy reference, bit for bit, up to counts."""
    nb = len(out["counts"])
    pu, nu = ctx.camera_download(nb)
    su = ctx.undistort_points(m, out["prev_pts"], out["counts"]); sn = ctx.undistort_points(m, out["next_pts"], out["counts"])
    for b in range(nb):
        n = int(out["counts"][b])
        assert n > 20, (tag, b, n)
        assert np.array_equal(bits(pu[b, :n]), bits(su[b, :n])) and np.array_equal(bits(nu[b, :n]), bits(sn[b, :n])), (tag, b)
        assert np.array_equal(bits(pu[b, :n]), bits(R.undistort_points(cam, out["prev_pts"][b, :n]))), (tag, b)
        assert np.array_equal(bits(nu[b, :n]), bits(R.undistort_points(cam, out["next_pts"][b, :n]))), (tag, b)
    return pu, nu


@pytest.mark.parametrize("streams,overlap", [(1, False), (1, True), (2, False), (2, True)])
def test_pairs_run_is_a_composition_of_stage_entries(pkg, ofk, streams, overlap):
    from of_amd.pipeline import FlowPipeline
    prev, nxt, sensors = pair_batch(pkg, ofk)
    cm, cam = pair_camera(ofk)
    tag = (streams, overlap)
    pipe = FlowPipeline(W, H, B, pair_cfg(), streams=streams)
    try:
        pipe.ctx.set_overlap(overlap)
        pipe.upload(prev, nxt, sensors)
        never = pipe.run()
        with pytest.raises(ofk.OfkError):
            pipe.ideal_points()
        pipe.ctx.set_camera(cm.setting())
        on = pipe.run()
        pu, nu = ideal_of_download(pipe.ctx, cm.setting(), cam, on, tag)
        again = pipe.run()                                       # the slices free-run over consecutive calls
        pipe.ctx.set_camera(None)
        off = pipe.run()
    finally:
        pipe.close()
    assert_image_side_identical(on, never, tag)
    assert_plain_records(on, pu, nu, sensors, tag)
    assert np.abs(on["records"][:, :3] - never["records"][:, :3]).max() > 1e-5       # the lens term reached the solve
    BO.assert_records_identical(again["records"], on["records"], tag)
    assert_image_side_identical(off, never, tag)
    BO.assert_records_identical(off["records"], never["records"], tag)


@pytest.mark.parametrize("setting", ["robust", "cov", "gate", "seed"])
def test_each_setting_with_the_camera_on(pkg, ofk, setting):
    from of_amd.pipeline import FlowPipeline
    prev, nxt, sensors = pair_batch(pkg, ofk)
    cm, cam = pair_camera(ofk)
    m = cm.setting()
    covd = dict(mode=cr.PROPAGATE, sigma_flow=0.3, sigma_pos=0.5, sigma_d=0.04, sigma_omega=(0.01, 0.02, 0.015), sigma_normal=0.004, sigma_offset=0.006,
                filter_r=False, r_floor=0.0, nis_max=0.0, omega_from_imu=False)
    cfg = {"robust": {}, "cov": dict(cov="propagate", sigma_flow_px=0.3, sigma_pos_px=0.5, sigma_d=0.04, sigma_omega=(0.01, 0.02, 0.015), sigma_normal=0.004,
                                     sigma_offset=0.006),
           "gate": dict(fb_check="seeded", fb_thr=0.05, fb_level=0, err_max=6.0), "seed": dict(lk_seed="model", seed_gain=1.0)}[setting]
    pipe = FlowPipeline(W, H, B, pair_cfg(**cfg), streams=2)
    try:
        if setting == "robust":
            pipe.ctx.set_robust(**ROBUST)
        pipe.upload(prev, nxt, sensors)
        off = pipe.run()
        pipe.ctx.set_camera(m)
        on = pipe.run()
        pu, nu = ideal_of_download(pipe.ctx, m, cam, on, setting)
        if setting == "robust":
            wts, st = pipe.ctx.robust_download(B)
        if setting == "cov":
            cov = pipe.covariances()
        if setting == "gate":
            stats = pipe.track_gate_stats()
        if setting == "seed":
            # the start positions: the predictor runs in the ideal image and its seeds come back through the lens
            seeds = pipe.ctx.distort_points(m, pipe.ctx.predict_points(pu, on["counts"], sensors, "model", 1.0), on["counts"])
            g0, g1 = pipe.ctx.gray_bgr8(prev), pipe.ctx.gray_bgr8(nxt)
            lk = pipe.ctx.lk_pyr(g0, g1, on["prev_pts"], on["counts"], win=15, max_level=3, max_count=20, eps=0.03, next_pts=seeds, flags=ofk.LK_USE_INITIAL_FLOW)
            raw_seeds = pipe.ctx.predict_points(on["prev_pts"], on["counts"], sensors, "model", 1.0)
    finally:
        pipe.close()
    if setting != "seed":
        assert_image_side_identical(on, off, setting)            # seeds differ with the camera: so may LK's end points
    else:
        assert np.array_equal(on["counts"], off["counts"]) and np.array_equal(bits(on["prev_pts"]), bits(off["prev_pts"]))
    assert np.abs(on["records"][:, :3] - off["records"][:, :3]).max() > 1e-5
    if setting in ("gate", "seed", "cov"):
        assert_plain_records(on, pu, nu, sensors, setting)
    if setting == "gate":
        assert stats[:, 0].min() > 20 and (stats[:, 1:].sum() > 0), stats           # the gates refused something, on the raw pixels
    for b in range(B):
        n = int(on["counts"][b]); sr = sensors[b]
        ok = on["status"][b, :n] == 1
        new = nu[b, :n].astype(np.float64); old = pu[b, :n].astype(np.float64)
        if setting == "robust":
            x = (new - [sr[20], sr[21]]) * sr[19]; u = (new - old) * sr[19]
            ref = robust_reference(b, x, u, ok, sr, st[b])
            np.testing.assert_allclose(on["records"][b, 0:3], ref["v"], rtol=0, atol=1e-10, err_msg=str(b))
            np.testing.assert_allclose(wts[b, :n], ref["weights"], rtol=0, atol=1e-9, err_msg=str(b))
            assert (wts[b, :n][ok] < 1.0).any()
        if setting == "cov":
            ref = cr.pair_record(cr.NODE, pu[b, :n], nu[b, :n], on["status"][b, :n], sr, covd, on["records"][b])
            assert ref[13] == 0 and cov[b, 13] == 0
            for sl in (slice(0, 6), slice(6, 12), slice(16, 22)):
                assert np.abs(cov[b, sl] - ref[sl]).max() <= 1e-9 * np.abs(ref[sl]).max(), (b, sl)
        if setting == "seed":
            for got, want in ((on["next_pts"], lk[0]), (on["status"], lk[1]), (on["err"], lk[2])):
                assert np.array_equal(bits(got[b, :n]), bits(want[b, :n])), b
            assert np.abs(seeds[b, :n] - raw_seeds[b, :n]).max() > 1e-3            # not the seeds the raw pixels would give


# ---------------------------------------------------------------------------------------------------- streams
FEAS_T = cc.FEAS_T
STREAM_CAM = dict(fx=640.0, fy=640.0, cx=320.0, cy=240.0, k=R.STRONG[1])
NSTEPS = 4


def stream_setup(pkg, ofk, kind="fused"):
    """The streams of tests/combined_cases.py with zones on.  The solve stage must reject points for the zones to have something to
    do: the plain step (whose feasibility rule leaves the status alone) drops the robust solve's zero-weight points, the fused steps
    drop what fails the feasibility rule."""
    from of_amd import synth
    from of_amd.pipeline import CameraModel, PipelineConfig
    frames, info = cc.sequences(synth)
    sensors = cc.sensor_rows(ofk, info)
    assert (info["scaling"], info["cx"], info["cy"]) == (1.0 / 640.0, 320.0, 240.0) == CameraModel(**STREAM_CAM).sensor_slots()
    cfg = PipelineConfig(**dict(cc.BASE, zones="hull", **(cc.ROBUST if kind == "step" else dict(use_feasibility=True, feas_T=FEAS_T))))
    return frames[:, :NSTEPS + 1], sensors, cfg, CameraModel(**STREAM_CAM), R.camera(R.BROWN, STREAM_CAM["k"], 640.0, 640.0, 320.0, 240.0)


def run_stream(ofk, kind, frames, sensors, cfg, camera):
    """The device's steps: per step dict(rec, tracks, counts, nxt, keep, zones, ideal)."""
    from of_amd.pipeline import FlowStream, FusionConfig
    fusion = None if kind == "step" else FusionConfig(use_imu=False, redetect_replace=kind == "replace")
    fs = FlowStream(cc.W, cc.H, batch=cc.NB, cfg=cfg, min_features=cc.MIN_FEAT, mask_radius=cc.RADIUS, fusion=fusion)
    try:
        if camera is not None:
            fs.ctx.set_camera(camera)
        tracks, counts = fs.begin(frames[:, 0])
        steps = [dict(tracks=tracks, counts=counts)]
        for t in range(1, frames.shape[1]):
            out = fs.step(frames[:, t], sensors) if kind == "step" else fs.step_fused(frames[:, t], sensors)
            nxt, keep = fs.ctx.stream_last_points(cfg.max_corners)
            steps.append(dict(rec=out[0], tracks=out[-2], counts=out[-1], nxt=nxt, keep=keep, zones=fs.zones(),
                              ideal=fs.ideal_points() if camera is not None else None))
        return steps
    finally:
        fs.close()


@pytest.mark.parametrize("kind", ["step", "fused", "replace"])
def test_stream_steps_with_zones_and_the_camera(pkg, ofk, sctx, kind):
    import robust_stream_oracle as rso
    frames, sensors, cfg, cm, cam = stream_setup(pkg, ofk, kind)
    on = run_stream(ofk, kind, frames, sensors, cfg, cm.setting())
    off = run_stream(ofk, kind, frames, sensors, cfg, None)
    m = cm.setting()
    ctx = sctx
    loops = [R.camera_loop(frames[b, 0], cfg, cc.MIN_FEAT, cc.RADIUS, cam, sensors[b],
                           rso.robust_solver(b, True, False) if kind == "step" else feasibility_solve(sensors[b, 22:25], FEAS_T, 2), zones={},
                           replace=kind == "replace") for b in range(cc.NB)]
    for b in range(cc.NB):
        assert np.array_equal(bits(on[0]["tracks"][b, :on[0]["counts"][b]]), bits(loops[b].tracks))
    inserted = masked = rejects = 0
    same = True                                                  # the image side equals the camera-off run's until the keep flags part
    for t in range(1, NSTEPS + 1):
        s, s_off = on[t], off[t]
        for b in range(cc.NB):
            tag = (kind, t, b)
            o = loops[b].step(frames[b, t], sensors[b])
            n = o["n_old"]
            assert kind != "step" or (o["gap"] >= 1e-6 and o["near"] == 0), tag      # no near-tie between two hypotheses: no allowance needed
            # the composition: the ideal points are the stage entry's of the raw ones the step tracked
            assert np.array_equal(bits(s["nxt"][b, :n]), bits(o["new"])), tag
            pu, nu = s["ideal"][0][b, :n], s["ideal"][1][b, :n]
            if n:
                assert np.array_equal(bits(pu), bits(ctx.undistort_points(m, o["old"]))) and np.array_equal(bits(nu), bits(ctx.undistort_points(m, s["nxt"][b, :n]))), tag
                assert np.array_equal(pu.astype(np.float64), o["ideal"][0]) and np.array_equal(nu.astype(np.float64), o["ideal"][1]), tag
            rec = s["rec"][b]
            assert rec[12] == n and rec[13] == o["n_tracked"] and rec[11] == o["used"] and s["counts"][b] == len(o["tracks"]), (tag, rec[11:14], o["used"])
            assert np.array_equal(s["keep"][b, :n] != 0, o["keep"]), tag
            assert np.array_equal(bits(s["tracks"][b, :s["counts"][b]]), bits(o["tracks"].astype(np.float32))), tag
            assert (o["v"] is not None) == o["solved"]
            if o["solved"]:
                np.testing.assert_allclose(rec[:3], o["v"], rtol=0, atol=1e-10, err_msg=str(tag))
                np.testing.assert_allclose(rec[8:11], o["v_uav"], rtol=0, atol=1e-10, err_msg=str(tag))
            z = o["zones"]
            assert np.array_equal(s["zones"]["stats"][b], z.stats), (tag, s["zones"]["stats"][b], z.stats)
            assert np.array_equal(s["zones"]["zones"][b], z.zones) and np.array_equal(bits(s["zones"]["motion"][b]), bits(z.motion)), tag
            inserted += int(z.stats[1]); rejects += int(z.stats[4]); masked += int(o["redetected"] and o["zones_masked"] > 0)
        if same:
            assert np.array_equal(bits(s["nxt"]), bits(s_off["nxt"])), (kind, t)            # same tracks in, same LK out
            same = np.array_equal(s["keep"], s_off["keep"])
            if same:
                assert np.array_equal(s["counts"], s_off["counts"]) and np.array_equal(bits(s["tracks"]), bits(s_off["tracks"])), (kind, t)
                for k in ("zones", "motion", "stats"):
                    assert np.array_equal(bits(s["zones"][k]), bits(s_off["zones"][k])), (kind, t, k)
                assert np.abs(s["rec"][:, :3] - s_off["rec"][:, :3]).max() > 1e-6        # and yet another solve
    print(f"{kind}: rejects {rejects}, zones inserted {inserted}, re-detections behind a zone mask {masked}, image side equal to camera off throughout: {same}")
    assert inserted > 0 and masked > 0 and rejects > 0


def test_off_equals_never_set(pkg, ofk):
    """A context that ran streams with the camera on (its ideal buffers exist) and had it switched off returns, from the next begin
    on, the bits of a context that never had the setting - for the plain and the fused step."""
    from of_amd.pipeline import FlowStream, FusionConfig
    for fused in (False, True):
        frames, sensors, cfg, cm, _ = stream_setup(pkg, ofk, "fused" if fused else "step")
        res = []
        for touch in (False, True):
            fs = FlowStream(cc.W, cc.H, batch=cc.NB, cfg=cfg, min_features=cc.MIN_FEAT, mask_radius=cc.RADIUS, fusion=FusionConfig(use_imu=False) if fused else None)
            step = (lambda t: fs.step_fused(frames[:, t], sensors)) if fused else (lambda t: fs.step(frames[:, t], sensors))
            try:
                if touch:
                    fs.ctx.set_camera(cm.setting())
                    fs.begin(frames[:, 0])
                    step(1); step(2)
                    fs.ideal_points()
                    fs.ctx.set_camera(None)
                    assert fs.ctx.get_camera().model == ofk.CAMERA_OFF
                    fs.ctx.zones_reset()
                fs.begin(frames[:, 0])
                res.append([tuple(step(t)) + tuple(fs.ctx.stream_last_points(cfg.max_corners)) + (fs.zones(),) for t in range(1, NSTEPS + 1)])
            finally:
                fs.close()
        for t, (x, y) in enumerate(zip(*res)):
            for i in range(len(x) - 1):
                assert np.array_equal(bits(x[i]), bits(y[i])), (fused, t, i)
            for k in ("zones", "motion", "stats"):
                assert np.array_equal(bits(x[-1][k]), bits(y[-1][k])), (fused, t, k)


# ---------------------------------------------------------------------------------------------------- the distorted scene
def test_rendered_scene_through_the_lens_on_the_device(pkg, ofk):
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    plain, lens, sr, cfg, cm, cam = R.scene_frames()
    s = R.SCENE
    chain = BO.oracle_chain(lens["prev"], lens["next"], cfg, sr)
    pipe = FlowPipeline(s["w"], s["h"], 2, PipelineConfig(**{**cfg.__dict__, "camera": cm}))
    try:
        pipe.upload(np.stack([lens["prev"], plain["prev"]]), np.stack([lens["next"], plain["next"]]), np.stack([sr, sr]))
        on = pipe.run()
        pu, nu = pipe.ideal_points()
        pipe.ctx.set_camera(None)
        off = pipe.run()
    finally:
        pipe.close()
    n = int(on["counts"][0])
    ref = dict(chain, v=R.solve_ideal(cam, chain, sr)[0])
    assert n == len(chain["pts"])
    for k, r in (("prev_pts", "pts"), ("next_pts", "nxt"), ("status", "status"), ("err", "err")):
        assert np.array_equal(bits(on[k][0, :n]), bits(chain[r])), k
    assert np.array_equal(bits(pu[0, :n]), bits(R.undistort_points(cam, chain["pts"]))) and np.array_equal(bits(nu[0, :n]), bits(R.undistort_points(cam, chain["nxt"])))
    np.testing.assert_allclose(on["records"][0, :3], ref["v"], rtol=0, atol=1e-10)
    BO.assert_pair_matches(off, 0, chain, "the lens frames, camera off")
    BO.assert_pair_matches(off, 1, BO.oracle_chain(plain["prev"], plain["next"], cfg, sr), "the frames without a lens")
    e_on, e_off, e_plain = R.rel_err(on["records"][0, :3]), R.rel_err(off["records"][0, :3]), R.rel_err(off["records"][1, :3])
    print("no lens", e_plain, "with the model", e_on, "without it", e_off)
    assert e_on <= 2.0 * e_plain and e_off >= 5.0 * e_plain, (e_plain, e_on, e_off)
