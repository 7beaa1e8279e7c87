"""The warp through a lens and the rectified view per stream on the device (ofk.h: ofk_warp_lens, ofk_set_rectify).

(a) k_warp_lens_u8 against its numpy restatement (tests/rectify_reference.py), frames and covered counts bit for bit: every matrix of
    stabilise_reference.matrices() (rounding ties, a W that changes sign, |fx| on either side of 2^30, NaN, inf, zero) taken as
    destination -> ideal pixel, plus M = NULL; Brown with tangential and rational terms, Brown without the rational terms (the skipped
    divide), the fisheye (whose inputs test_rectify_reference.py shows to be free of rounding ties), a denominator that crosses zero
    inside the frame, r_max binding inside the frame; fo_x != fo_y; sizes from 1 x 1 to 240 x 320 with a destination that differs
    from the source (4 k + 1 rows, widths 254 / 256 / 258: the second block column and the byte stores); both channel counts, both
    borders; batches of 1, 3 and 65.
(b) Two lens-rendered 12-frame streams through FlowStream with camera, track table, finite motion, keyframe (max_age = 3), view and
    rectify: every step's frame and cover are ofk_warp_lens's on the downloaded M with the context's camera, every pose record
    ofk_stab_pose's on the downloads, everything else the bits of the run with view and rectify off; the gain over the raw frames.
(c) Refusals and inertness.  (d) The cv2_hip functions are the stage entry."""
import numpy as np
import pytest

import camera_reference as cr
import rectify_reference as rr
import stabilise_reference as sr
import test_gpu_stabilise as tgs
from test_gpu_keyframe import bits, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(ofk):
    c = ofk.Context(0, 320, 240, 65, 16, 2)
    yield c
    c.close()


def device_camera(ofk, cam):
    return ofk.Camera(cam["model"], cam["iters"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], (ofk.C.c_double * 8)(*cam["k"]), cam["fo_x"], cam["fo_y"],
                      cam["co_x"], cam["co_y"])


def check(ctx, ofk, src, M, cam, dsize, border, bval, r_max, tag):
    got, cov = ctx.warp_lens(src, device_camera(ofk, cam), M, dsize, border, bval, r_max)
    want, wcov, tie = rr.warp_lens_batch(src, M, cam, dsize, border, bval, r_max)
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = [b for b in range(len(src)) if not np.array_equal(got[b], want[b])]
    assert not bad, (tag, bad, [int(np.count_nonzero(got[b] != want[b])) for b in bad])
    assert np.array_equal(cov, wcov), (tag, cov, wcov)
    return got, cov, tie


@pytest.mark.parametrize("ch", (1, 3))
@pytest.mark.parametrize("border,bval", ((sr.BORDER_CONSTANT, 200), (sr.BORDER_REPLICATE, 0)))
@pytest.mark.parametrize("ssize,dsize", rr.PAIRS)
def test_every_matrix_and_lens_bit_for_bit(ctx, ofk, ssize, dsize, ch, border, bval):
    """One batch per lens: every matrix of matrices() over its own random image; then the batch once more with M = NULL."""
    mats = sr.matrices(*ssize, *dsize)
    names = list(mats)
    M = np.stack(list(mats.values()))
    src = np.stack([tgs.image(*ssize, ch, 100 + k) for k in range(len(M))])
    seen = {}
    for lens, (cam, r_max) in rr.cameras(*ssize).items():
        got, cov, tie = check(ctx, ofk, src, M, cam, dsize, border, bval, r_max, (lens, ssize, dsize))
        assert lens != "fisheye" or tie >= rr.FISH_TIE
        for name in ("nan", "inf", "nan_in_w"):                   # nothing is inside: the border value everywhere, under either border
            assert cov[names.index(name)] == 0
        assert np.all(got[names.index("nan_in_w")] == bval)
        check(ctx, ofk, src[:3], None, cam, dsize, border, bval, r_max, (lens, ssize, dsize, "NULL"))
        seen[lens] = (got[names.index("identity")], cov[names.index("identity")])
    if ssize == dsize == (240, 320):                              # the lenses differ; r_max takes pixels out of the view; the pole lies inside it
        assert not np.array_equal(seen["rational"][0], seen["poly"][0]) and not np.array_equal(seen["pole"][0], seen["poly"][0])
        assert seen["r_max"][1] < seen["poly"][1] and np.count_nonzero(seen["r_max"][0] != seen["poly"][0]) > 1000
        pole = rr.cameras(*ssize)["pole"][0]
        x, y = (np.arange(320.0)[None, :] - pole["co_x"]) / pole["fo_x"], (np.arange(240.0)[:, None] - pole["co_y"]) / pole["fo_y"]
        den = 1.0 + pole["k"][5] * (x * x + y * y)
        assert den.min() < 0.0 < den.max() and np.abs(den).min() < 1e-3


@pytest.mark.parametrize("batch", (1, 3, 65))
@pytest.mark.parametrize("ch", (1, 3))
def test_batches_of_distinct_matrices(ctx, ofk, batch, ch):
    rng = np.random.default_rng(7 + batch)
    ssize, dsize = (67, 33), (64, 16)
    M = np.empty((batch, 3, 3))
    for b in range(batch):
        a = rng.uniform(-0.2, 0.2)
        M[b] = [[np.cos(a), -np.sin(a), rng.uniform(-8, 8)], [np.sin(a), np.cos(a), rng.uniform(-8, 8)], [rng.uniform(-2e-4, 2e-4), rng.uniform(-2e-4, 2e-4), 1.0]]
    src = np.stack([tgs.image(*ssize, ch, 300 + b) for b in range(batch)])
    for lens in ("rational", "poly", "fisheye"):
        cam, r_max = rr.cameras(*ssize)[lens]
        _, cov, tie = check(ctx, ofk, src, M, cam, dsize, sr.BORDER_CONSTANT, 0, r_max, (lens, batch))
        assert lens != "fisheye" or tie >= rr.FISH_TIE
        assert len(set(cov.tolist())) > 1 or batch == 1


def test_single_image_stage_wrapper_and_cv2_facade(ctx, pkg, ofk):
    from of_amd import cv2_hip, velocity_node
    from of_amd.pipeline import CameraModel
    h, w = 33, 67
    gray, bgr = tgs.image(h, w, 1, 1), tgs.image(h, w, 3, 2)
    K = np.array([[60.0, 0, 33.2], [0, 61.0, 16.4], [0, 0, 1.0]])
    Knew = np.array([[50.0, 0, 30.0], [0, 52.0, 15.0], [0, 0, 1.0]])
    D = np.array([-0.28, 0.09, 0.0008, -0.0005, -0.012])
    brown = cr.camera(cr.BROWN, D, 60.0, 61.0, 33.2, 16.4, fo_x=60.0, fo_y=61.0)
    brown_new = cr.camera(cr.BROWN, D, 60.0, 61.0, 33.2, 16.4, fo_x=50.0, fo_y=52.0, co_x=30.0, co_y=15.0)
    got, cov = ctx.warp_lens(gray, device_camera(ofk, brown), None)
    want, mask, _ = rr.warp_lens(gray, None, brown)
    assert np.array_equal(got, want) and cov == np.count_nonzero(mask) and isinstance(cov, int)
    assert np.array_equal(cv2_hip.undistort(gray, K, D), want)
    dst = np.zeros_like(gray)
    assert cv2_hip.undistort(gray, K, D, dst) is dst and np.array_equal(dst, want)      # a dst of the right shape is filled in place
    assert np.array_equal(cv2_hip.undistort(bgr, K, D, newCameraMatrix=Knew), ctx.warp_lens(bgr, device_camera(ofk, brown_new), None)[0])
    assert np.array_equal(cv2_hip.undistort(bgr, K, D, newCameraMatrix=Knew), rr.warp_lens(bgr, None, brown_new)[0])
    Df = np.array([-0.03, 0.005, -0.001, 0.0002])
    fish = cr.camera(cr.FISHEYE, Df, 60.0, 61.0, 33.2, 16.4, fo_x=50.0, fo_y=52.0, co_x=30.0, co_y=15.0)
    a = cv2_hip.fisheye.undistortImage(bgr, K, Df, Knew=Knew, new_size=(40, 30))
    b, _ = ctx.warp_lens(bgr, device_camera(ofk, fish), None, (30, 40))
    assert a.shape == (30, 40, 3) and np.array_equal(a, b)
    wf, _, tie = rr.warp_lens(bgr, None, fish, (30, 40))
    assert tie.min() >= rr.FISH_TIE and np.array_equal(a, wf)
    M = sr.matrices(h, w, 30, 40)["rotation"]
    cm = CameraModel(fx=60.0, fy=61.0, cx=33.2, cy=16.4, k=tuple(D), fo=60.0)
    one = cr.camera(cr.BROWN, D, 60.0, 61.0, 33.2, 16.4)
    f, c = velocity_node.rectify_frame(gray, cm, M, (30, 40), "replicate", 0, r_max=0.4)
    wf, wm, _ = rr.warp_lens(gray, M, one, (30, 40), sr.BORDER_REPLICATE, 0, 0.4)
    assert np.array_equal(f, wf) and c == np.count_nonzero(wm)


def test_stage_entry_refusals(ctx, ofk):
    src, cam = tgs.image(8, 8, 1, 3), device_camera(ofk, rr.cameras(8, 8)["poly"][0])
    for kw in (dict(border=2), dict(border_value=256), dict(border_value=-1), dict(dsize=(241, 320)), dict(r_max=-1.0), dict(r_max=float("nan")),
               dict(r_max=float("inf"))):
        with pytest.raises(ofk.OfkError) as e:
            ctx.warp_lens(src, cam, np.eye(3), **kw)
        assert e.value.code == ofk.E_INVALID, kw
    off = device_camera(ofk, dict(rr.cameras(8, 8)["poly"][0], model=0))
    zero_f = device_camera(ofk, dict(rr.cameras(8, 8)["poly"][0], fo_y=0.0))
    for bad in (off, zero_f):
        with pytest.raises(ofk.OfkError) as e:
            ctx.warp_lens(src, bad)
        assert e.value.code == ofk.E_INVALID
    L = ofk.load_library()
    out = np.zeros((8, 8, 2), np.uint8)
    assert L.ofk_warp_lens(ctx._h, ofk.C.byref(cam), ofk._p(out), 8, 8, 2, None, ofk._p(out), 8, 8, 0, 0, 0.0, 1, None) == ofk.E_INVALID
    assert L.ofk_warp_lens(ctx._h, None, ofk._p(src), 8, 8, 1, None, ofk._p(out), 8, 8, 0, 0, 0.0, 1, None) == ofk.E_INVALID
    got, cov = ctx.warp_lens(src, cam)                              # and the context still works
    assert np.array_equal(got, rr.warp_lens(src, None, rr.cameras(8, 8)["poly"][0])[0])


# ------------------------------------------------------------------------------------------------ the rectified view in the stream steps
SH, SW, SNF, NB = tgs.SH, tgs.SW, tgs.SNF, tgs.NB
LENS_CHAIN_GAIN = 21.4                                           # tests/test_rectify_reference.py: the CPU chain's smallest gain behind a lens
_seq = {}


def lens_streams(pkg, lens):
    """Two streams, one per motion, seen through `lens`: BGR frames [2, 12, 240, 320, 3], the sensor rows, the camera (dict, CameraModel)."""
    if lens not in _seq:
        import of_amd.ofk as ofk
        from of_amd.pipeline import CameraModel
        frames, sensors = [], []
        for which in range(NB):
            _, _, _, cam, f, info = rr.lens_sequence(which, lens, SNF)
            frames.append(f)
            sensors.append(ofk.make_sensors(1, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"],
                                            v_prior=info["v"])[0])
        _seq[lens] = (np.stack(frames), np.stack(sensors), cam, CameraModel(**rr.seq_camera(rr.LENSES[lens])[1]))
    return _seq[lens]


def run_lens(pkg, ofk, lens, view_on, r_max=0.0):
    """ofk_stream_step_fused over the lens-rendered streams, no re-detection, max_age = 3.  -> (what the calls returned, per step (rec,
    covered, frames))."""
    from of_amd.pipeline import FlowStream, FusionConfig
    frames, sensors, cam, cm = lens_streams(pkg, lens)
    s = sr.setting()
    cfg = tgs.stab_cfg("fused", tgs.device_stab(ofk, s) if view_on else None, 3, camera=cm, rectify=ofk.rectify_setting(r_max=r_max) if view_on else None)
    fusion = FusionConfig()
    fs = FlowStream(SW, SH, batch=NB, cfg=cfg, min_features=0, mask_radius=tgs.SRADIUS, fusion=fusion)
    ctx, side = fs.ctx, ofk.Context(0, SW, SH, NB, 16, 1)
    out, views, state, prev_cov = [], [], None, None
    try:
        assert ctx.get_rectify().mode == (1 if view_on else 0) and ctx.get_camera().model == cam["model"]
        ctx.imu_reset(NB)
        tracks, counts = ctx.stream_begin(frames[:, 0], cfg.to_params())
        for t in range(1, SNF):
            rec, fz, tracks, counts = ctx.stream_step_fused(frames[:, t], sensors, cfg.to_params(), fusion.to_struct(), 0, tgs.SRADIUS)
            kd = ctx.keyframe_download(NB, tgs.SMC)
            out.append((rec.copy(), tracks.copy(), counts.copy(), ctx.track_table_download(NB, tgs.SMC), {k: kd[k] for k in ("R_acc", "rec")}, fz.copy()))
            if not view_on:
                continue
            d = ctx.stab_download(NB, SH, SW)
            views.append((d["rec"].copy(), d["covered"].copy(), d["frames"].copy()))
            R_used = d["rec"][:, 18:27].reshape(NB, 3, 3)
            pc = np.zeros(NB, np.int32) if prev_cov is None else prev_cov
            state, got_rec = side.stab_pose(R_used, kd["rec"], sensors, SH, SW, state=state, prev_covered=pc, stabilise=tgs.device_stab(ofk, s))
            assert np.array_equal(bits(got_rec), bits(d["rec"])), (lens, t, "the step's record is ofk_stab_pose's on the downloads")
            prev_cov = d["covered"].copy()
            gray = np.stack([ctx.resident_pyramid(0, b, SH, SW, 0)[0] for b in range(NB)])       # the step's new RAW frame, as the warp read it
            wf, wc = side.warp_lens(gray, ctx.get_camera(), d["rec"][:, 0:9].reshape(NB, 3, 3), None, s["border"], s["border_value"], r_max)
            assert np.array_equal(wf, d["frames"]) and np.array_equal(wc, d["covered"]), (lens, t, "the frame is ofk_warp_lens's on the downloaded M")
            if lens == "STRONG":                                 # Brown: the restatement's too
                rf, rc, _ = rr.warp_lens_batch(gray, d["rec"][:, 0:9].reshape(NB, 3, 3), cam, None, s["border"], s["border_value"], r_max)
                assert np.array_equal(rf, d["frames"]) and np.array_equal(rc, d["covered"]), (lens, t)
    finally:
        fs.close(); side.close()
    return out, views


@pytest.mark.parametrize("lens", ("STRONG", "FISH"))
def test_rectified_view_chained_over_rekeys_holds_the_ground_still(pkg, ofk, lens):
    """Measured on the device, smallest raw / stabilised mean abs diff over both streams: 19.1 behind the Brown lens, 21.4 behind the
    fisheye (CPU chain 21.4 - 24.1); asserted at half the CPU chain's smallest figure behind a lens."""
    from of_amd.pipeline import CameraModel
    frames, _, cam, cm = lens_streams(pkg, lens)
    r_max = 1.05 * cm.ideal_radius(SH, SW)
    on, views = run_lens(pkg, ofk, lens, True, r_max)
    off, _ = run_lens(pkg, ofk, lens, False)
    same(on, off, (lens, "view and rectify on against off"))
    assert np.all(views[0][0][:, 30] == sr.NONE)                 # the first step finds no keyframe: the frame is rectified and no more
    assert np.all(views[-1][0][:, 30] == sr.FULL) and np.all(views[-1][0][:, 33] == 0)
    assert min(int(np.sum([v[0][b, 35] for v in views])) for b in range(NB)) >= 3
    gray = rr.gray_of(frames)
    g = []
    for b in range(NB):
        ref = views[0][2][b].astype(np.int32)
        for k, (rec, cov, fr) in enumerate(views[1:], 2):
            mask = rr.warp_lens(gray[b, k], rec[b, 0:9].reshape(3, 3), cam, None, sr.BORDER_CONSTANT, 0, r_max)[1]
            assert cov[b] == np.count_nonzero(mask) or lens == "FISH"
            stab = np.abs(fr[b].astype(np.int32) - ref)[mask].mean()
            raw = np.abs(gray[b, k].astype(np.int32) - gray[b, 1].astype(np.int32)).mean()
            g.append(raw / stab)
    print(lens, "device gain, smallest over both streams", min(g), "CPU chain", LENS_CHAIN_GAIN)
    assert min(g) >= LENS_CHAIN_GAIN / 2.0, g


def test_refusals_and_inertness(pkg, ofk):
    from of_amd.pipeline import CameraModel
    frames, sensors = tgs.stream_frames(pkg)
    cfg = tgs.stab_cfg("fused", None)
    cam = CameraModel(fx=320.0, fy=320.0, cx=160.0, cy=120.0, k=(-0.1, 0.01, 0, 0)).setting()

    def run(prepare, steps=(1, 2, 3)):
        ctx = ofk.Context(0, SW, SH, NB, tgs.SMC, cfg.max_level)
        try:
            ctx.set_track_table(ofk.track_table_setting())
            ctx.set_keyframe(ofk.keyframe_setting(max_age=1))
            ctx.set_stabilise(ofk.stabilise_setting())
            prepare(ctx)
            ctx.stream_begin(frames[:, 0], cfg.to_params())
            for t in steps:
                ctx.stream_step(frames[:, t], sensors, cfg.to_params(), 0, tgs.SRADIUS)
            d = ctx.stab_download(NB, SH, SW)
            return d["frames"], d["covered"], d["rec"]
        finally:
            ctx.close()

    def refused(prepare, name):
        with pytest.raises(ofk.OfkError) as e:
            run(prepare, (1,))
        assert e.value.code == ofk.E_INVALID and name in str(e.value), (name, str(e.value))

    refused(lambda c: c.set_camera(cam), "ofk_set_camera")                                          # rectify off: as it always was
    refused(lambda c: (c.set_rectify(ofk.rectify_setting()), c.set_rectify(None), c.set_camera(cam)), "ofk_set_camera")
    rs = ofk.rshutter_setting("flow", readout=0.6, anchor=0.4)
    refused(lambda c: (c.set_rectify(ofk.rectify_setting()), c.set_rolling_shutter(rs)), "ofk_set_rolling_shutter")
    refused(lambda c: (c.set_rectify(ofk.rectify_setting()), c.set_camera(cam), c.set_rolling_shutter(rs)), "ofk_set_rolling_shutter")
    never = run(lambda c: None)
    inert = run(lambda c: c.set_rectify(ofk.rectify_setting(r_max=0.01)))                          # no camera: the plain warp runs
    off_again = run(lambda c: (c.set_rectify(ofk.rectify_setting(r_max=0.01)), c.set_rectify(None)))
    for other in (inert, off_again):
        assert np.array_equal(other[0], never[0]) and np.array_equal(other[1], never[1]) and np.array_equal(bits(other[2]), bits(never[2]))
    ctx = ofk.Context(0, 64, 48, 2, 100, 2)
    try:                                                          # the setting round-trips; every refusal leaves it as it was
        assert (ctx.get_rectify().mode, ctx.get_rectify().r_max) == (0, 0.0)
        ctx.set_rectify(ofk.Rectify(1, 1.25))
        for bad in (ofk.Rectify(2, 0.0), ofk.Rectify(-1, 0.0), ofk.Rectify(1, -0.5), ofk.Rectify(1, float("nan")), ofk.Rectify(1, float("inf"))):
            with pytest.raises(ofk.OfkError) as e:
                ctx.set_rectify(bad)
            assert e.value.code == ofk.E_INVALID and (ctx.get_rectify().mode, ctx.get_rectify().r_max) == (1, 1.25)
        ctx.set_rectify(ofk.Rectify(0, -9.0))                      # mode off: off, whatever else it holds
        assert (ctx.get_rectify().mode, ctx.get_rectify().r_max) == (0, 1.25)
    finally:
        ctx.close()
