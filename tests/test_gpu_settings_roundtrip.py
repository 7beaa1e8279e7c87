"""What the seventeen struct settings and the three point corrections promise at the C boundary (include/ofk.h), pinned byte for byte.

Every ofk_set_* / ofk_get_* pair: get after a valid set returns the same bytes; NULL switches the setting off the way that setter
does it (they differ: which fields are cleared, whether a struct whose mode is OFF counts as NULL); an invalid struct is refused with
OFK_E_INVALID and the message written out below, and leaves the setting as it was.  The point corrections: the setter's and the stage
entry's rules where they differ, the downloads before and after a run (host pitch, truncation, untouched bytes, one NULL pointer), and
the stage entries' refusal of counts outside 0..stride."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W, B, PTS = 48, 64, 2, 16
SENTINEL = np.float32(-7.5)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.fixture(scope="module")
def ctx(ofk):
    c = ofk.Context(0, W, H, B, PTS, 1)
    yield c
    c.close()


def d3(a, b, c):
    return (C.c_double * 3)(a, b, c)


def cases(ofk):
    """name -> (struct class, a valid struct, an invalid one, its message, what NULL clears as {field: value})."""
    k8 = (C.c_double * 8)(-0.1, 0.02, 1e-3, -1e-3, 0, 0, 0, 0)
    return {
        "robust": (ofk.Robust, ofk.Robust(ofk.ROBUST_HUBER, 1.5, 7, 33, 0x123456789ABCDEF0, 1), ofk.Robust(7, 1.5, 7, 33, 5, 1),
                   "ofk_set_robust: loss 7 is neither OFK_ROBUST_HUBER nor _TUKEY", dict(loss=0)),
        "cov": (ofk.Cov, ofk.Cov(ofk.COV_RESIDUAL, 0.1, 0.2, 0.3, d3(0.4, 0.5, 0.6), 0.7, 0.8, 1, 1, 0.9, 11.0),
                ofk.Cov(9, 0.1, 0.2, 0.3, d3(0.4, 0.5, 0.6), 0.7, 0.8, 1, 1, 0.9, 11.0),
                "ofk_set_cov: mode 9 is none of OFK_COV_OFF, _PROPAGATE, _RESIDUAL", dict(mode=0, filter_r=0)),
        "joint": (ofk.Joint, ofk.Joint(1, 0.3, d3(0.0, np.inf, 2.0), 1), ofk.Joint(1, 0.0, d3(0.0, np.inf, 2.0), 1),
                  "ofk_set_joint: sigma_flow 0 is not finite or not positive", dict(mode=0)),
        "plane": (ofk.Plane, ofk.Plane(1, 0.3, np.inf, 0.05, d3(0.1, 0.2, 0.9), 9), ofk.Plane(1, 0.3, np.inf, 0.05, d3(0.1, 0.2, 0.9), 0),
                  "ofk_set_plane: iters 0 is outside 1..16", dict(mode=0)),
        "epipolar": (ofk.Epipolar, ofk.Epipolar(1, 55.0, 7, 0.01, d3(0.1, 0.2, 0.9), ofk.EPI_W_ROBUST),
                     ofk.Epipolar(1, 55.0, 0, 0.01, d3(0.1, 0.2, 0.9), ofk.EPI_W_ROBUST), "ofk_set_epipolar: anchor_min 0 is below 1", dict(mode=0)),
        "track_gate": (ofk.TrackGate, ofk.TrackGate(ofk.FB_SEEDED, 0.75, 1, 12.5), ofk.TrackGate(ofk.FB_SEEDED, 0.75, 5, 12.5),
                       "ofk_set_track_gate: fb_level 5 outside -1..1", dict(fb_mode=0, err_max=0.0)),
        "corner_grid": (ofk.CornerGrid, ofk.CornerGrid(8, 3, 100), ofk.CornerGrid(8, 0, 100),
                        "ofk_set_corner_grid: corner grid cap 0 must be at least 1", dict(cell=0)),
        "zones": (ofk.Zones, ofk.Zones(ofk.ZONES_HULL, 40, 4, 17, 25, 9), ofk.Zones(ofk.ZONES_HULL, 40, 17, 17, 25, 9),
                  "ofk_set_zones: min_members 17 outside 1..16", dict(mode=0)),
        "camera": (ofk.Camera, ofk.Camera(ofk.CAMERA_BROWN, 12, 60.0, 61.0, 32.0, 24.0, k8, 160.0, 160.0, 33.0, 25.0),
                   ofk.Camera(ofk.CAMERA_BROWN, 12, 60.0, 61.0, 32.0, 24.0, k8, 160.0, 150.0, 33.0, 25.0),
                   "ofk_set_camera: fo_x = 160 and fo_y = 150 differ: the solve has one scaling (sensors[19] = 1 / fo_x)", dict(model=0)),
        "rolling_shutter": (ofk.RShutter, ofk.RShutter(ofk.RS_GYRO, 0, -0.75, 0.25, 2.0), ofk.RShutter(ofk.RS_GYRO, 0, 1.5, 0.25, 2.0),
                            "ofk_set_rolling_shutter: readout 1.5 outside -1..1 frame intervals", dict(mode=0)),
        "finite_motion": (ofk.FiniteMotion, ofk.FiniteMotion(ofk.FM_EXACT, 0.25), ofk.FiniteMotion(ofk.FM_EXACT, 2.0),
                          "ofk_set_finite_motion: min_depth 2 outside (0, 1]", dict(mode=0)),
        "gyro_bias": (ofk.GyroBias, ofk.GyroBias(1, 0.3, 2e-5, 1e-12, d3(1e-2, 0.0, 1e4), d3(1e-3, -2e-3, 0.0), 9.5, 1),
                      ofk.GyroBias(1, 0.3, 2e-5, 1e-12, d3(1e-2, 1e160, 1e4), d3(1e-3, -2e-3, 0.0), 9.5, 1),
                      "ofk_set_gyro_bias: the square of p0[1] is not finite (1e+160)", dict(mode=0)),
        "track_table": (ofk.TrackTable, ofk.TrackTable(ofk.TT_ON, ofk.TT_SEED_FLOW, 0.75), ofk.TrackTable(ofk.TT_ON, 5, 0.75),
                        "ofk_set_track_table: seed 5 is neither OFK_TT_SEED_OFF nor OFK_TT_SEED_FLOW", dict(mode=0)),
        "track_depth": (ofk.TrackDepth, ofk.TrackDepth(1, 0.3, 0.25, 2.5, 1e-6, 4, 0.3, 9, 0), ofk.TrackDepth(1, 0.3, 0.25, 2.5, 1e-6, 4, 0.3, 2, 0),
                        "ofk_set_track_depth: min_rows = 2 must be at least 3", dict(mode=0)),
        "track_template": (ofk.TrackTemplate, ofk.TrackTemplate(1, 9, 0.7, 2, 1.5, ofk.TPL_DROP, 7, 1.5, 1.25),
                           ofk.TrackTemplate(1, 4, 0.7, 2, 1.5, ofk.TPL_DROP, 7, 1.5, 1.25),
                           "ofk_set_track_template: win = 4 must be odd and in 5..31", dict(mode=0)),
        "keyframe": (ofk.Keyframe, ofk.Keyframe(1, 0.3, 1.5, 9, 0.25, 0.4, 12), ofk.Keyframe(1, 0.3, 1.5, 9, 1.5, 0.4, 12),
                     "ofk_set_keyframe: min_share = 1.5 outside [0, 1]", dict(mode=0)),
        "keyframe_rotation": (ofk.KeyframeRotation, ofk.KeyframeRotation(1, ofk.KEYROT_ATTITUDE, (C.c_int * 3)(1, 0, 1), 1e-3, 2e-4, 3e-3, 3, 0.05),
                              ofk.KeyframeRotation(1, ofk.KEYROT_ATTITUDE, (C.c_int * 3)(1, 0, 1), 1e-3, 2e-4, 3e-3, 9, 0.05),
                              "ofk_set_keyframe_rotation: iters = 9 outside 1..8", dict(mode=0)),    # 8: OFK_KEYROT_MAX_ITERS
    }


NAMES = ["robust", "cov", "joint", "plane", "epipolar", "track_gate", "corner_grid", "zones", "camera", "rolling_shutter", "finite_motion", "gyro_bias",
         "track_table", "track_depth", "track_template", "keyframe", "keyframe_rotation"]
OFF_IS_NULL = ("robust", "camera", "rolling_shutter", "finite_motion", "gyro_bias", "track_table", "track_depth", "track_template", "keyframe",
               "keyframe_rotation")       # a struct whose mode is OFF is not read beyond the mode
OFF_IS_COPIED = ("joint", "plane", "epipolar")                                 # ... is checked and copied whole


def clone(s):
    return type(s).from_buffer_copy(bytes(s))


def with_fields(s, fields):
    s = clone(s)
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def refused(ofk, call, message):
    with pytest.raises(ofk.OfkError) as e:
        call()
    assert e.value.code == ofk.E_INVALID and str(e.value) == f"libofk error {ofk.E_INVALID}: {message}", str(e.value)


@pytest.mark.parametrize("name", NAMES)
def test_set_get_off_and_refusal(ofk, ctx, name):
    cls, valid, invalid, message, cleared = cases(ofk)[name]
    setter, getter = getattr(ctx, "set_" + name), getattr(ctx, "get_" + name)
    try:
        setter(valid)
        got = getter()
        assert isinstance(got, cls) and bytes(got) == bytes(valid)
        refused(ofk, lambda: setter(invalid), message)
        assert bytes(getter()) == bytes(valid)                   # a refused struct leaves the setting as it was
        setter(None)
        off = with_fields(valid, cleared)
        assert bytes(getter()) == bytes(off) and bytes(off) != bytes(valid)
        # a struct whose mode field is OFF
        mode = next(iter(cleared))
        setter(valid)
        if name in OFF_IS_NULL:                                  # NULL's path: nothing else of the struct is looked at or kept
            junk = cls.from_buffer_copy(b"\xff" * C.sizeof(cls)); setattr(junk, mode, 0)
            setter(junk)
            assert bytes(getter()) == bytes(off)
        elif name in OFF_IS_COPIED:                              # checked like any other, then copied whole
            other = with_fields(invalid, {mode: 0})
            refused(ofk, lambda: setter(other), message)
            assert bytes(getter()) == bytes(valid)
            other = with_fields(valid, {mode: 0, "beam" if name != "joint" else "sigma_omega": d3(3.0, 4.0, 5.0)})
            setter(other)
            assert bytes(getter()) == bytes(other) and bytes(other) != bytes(off)
        elif name == "cov":                                      # checked (filter_r needs a mode), copied whole
            refused(ofk, lambda: setter(with_fields(valid, dict(mode=0))), "ofk_set_cov: filter_r needs a covariance: mode is OFK_COV_OFF")
            other = with_fields(valid, dict(mode=0, filter_r=0, sigma_d=7.0))
            setter(other)
            assert bytes(getter()) == bytes(other)
        elif name == "track_gate":                               # fb off with the err cap on is a gate of its own: copied whole
            other = with_fields(valid, dict(fb_mode=0, fb_thr=-1.0))
            setter(other)
            assert bytes(getter()) == bytes(other)
        elif name == "corner_grid":                              # cell 0: the other fields are not checked, the struct is copied whole
            other = ofk.CornerGrid(0, -5, -6)
            setter(other)
            assert bytes(getter()) == bytes(other)
        elif name == "zones":                                    # only the mode is checked and only the mode is written
            setter(ofk.Zones(ofk.ZONES_OFF, -1, -2, -3, -4, -5))
            assert bytes(getter()) == bytes(off)
    finally:
        setter(None)


def test_keywords_reach_the_setting_makers(ofk, ctx):
    """set_X(**settings) builds the struct with X_setting; set_X() without either is NULL."""
    try:
        ctx.set_finite_motion(min_depth=0.5)
        assert bytes(ctx.get_finite_motion()) == bytes(ofk.finite_motion_setting(min_depth=0.5))
        ctx.set_finite_motion()
        assert ctx.get_finite_motion().mode == ofk.FM_OFF and ctx.get_finite_motion().min_depth == 0.5
        ctx.set_cov(mode="residual", sigma_flow=0.25)
        assert bytes(ctx.get_cov()) == bytes(ofk.cov_setting(mode="residual", sigma_flow=0.25))
        ctx.set_zones(link=12)
        assert bytes(ctx.get_zones()) == bytes(ofk.zones_setting(link=12))
    finally:
        ctx.set_finite_motion(None); ctx.set_cov(None); ctx.set_zones(None)


def test_null_struct_pointer_to_a_getter(ofk, ctx):
    for name in NAMES:
        assert getattr(ctx._L, "ofk_get_" + name)(ctx._h, None) == ofk.E_INVALID, name
        assert getattr(ctx._L, "ofk_set_" + name)(None, None) == ofk.E_INVALID, name


# ---------------------------------------------------------------------------------------------------- setter rule / stage rule
def stage_arrays():
    rng = np.random.default_rng(3)
    p0 = rng.uniform(4.0, 44.0, (B, 4, 2)).astype(np.float32)
    return p0, p0 + np.float32(0.75)


def sensors_of(ofk):
    return ofk.make_sensors(B, d=1.0, omega=(0.004, -0.003, 0.004), offset=(0.02, -0.01, 0.2), scaling=1.0 / 60.0, cx=W / 2.0, cy=H / 2.0, v_prior=(0.02, -0.03, 0.01))


def test_camera_two_focal_lengths(ofk, ctx):
    _, _, two_focal, message, _ = cases(ofk)["camera"]
    refused(ofk, lambda: ctx.set_camera(two_focal), message)
    p0, _ = stage_arrays()
    out = ctx.undistort_points(two_focal, p0)
    assert out.shape == p0.shape and np.isfinite(out).all() and not np.array_equal(out, p0)
    back = ctx.distort_points(ofk.Camera.from_buffer_copy(bytes(two_focal)), out)
    assert np.abs(back - p0).max() < 1e-3


def test_rolling_shutter_rows_zero(ofk, ctx):
    rs = ofk.RShutter(ofk.RS_FLOW, 0, 0.5, 0.5, 1.0)
    p0, p1 = stage_arrays()
    try:
        ctx.set_rolling_shutter(rs)
        assert bytes(ctx.get_rolling_shutter()) == bytes(rs)
    finally:
        ctx.set_rolling_shutter(None)
    refused(ofk, lambda: ctx.rs_correct_points(rs, p0, p1), "ofk_rs_correct_points: rows 0 means the frame height of a run: the stage entry needs rows > 0")
    rs.rows = H
    a, b = ctx.rs_correct_points(rs, p0, p1)
    assert np.isfinite(a).all() and not np.array_equal(b, p1)


@pytest.mark.parametrize("entry", ["ofk_undistort_points", "ofk_distort_points", "ofk_rs_correct_points", "ofk_finite_correct_points"])
def test_stage_entries_refuse_counts_outside_the_stride(ofk, ctx, entry):
    p0, p1 = stage_arrays()
    cam = cases(ofk)["camera"][1]
    call = {"ofk_undistort_points": lambda n: ctx.undistort_points(cam, p0, n),
            "ofk_distort_points": lambda n: ctx.distort_points(cam, p0, n),
            "ofk_rs_correct_points": lambda n: ctx.rs_correct_points(ofk.RShutter(ofk.RS_GYRO, H, 0.5, 0.5, 1.0), p0, p1, n, sensors=sensors_of(ofk)),
            "ofk_finite_correct_points": lambda n: ctx.finite_correct_points(ofk.FiniteMotion(ofk.FM_EXACT, 0.1), p0, p1, n, sensors=sensors_of(ofk))}[entry]
    refused(ofk, lambda: call((1, 5)), f"{entry}: counts[1]=5 outside 0..4")
    refused(ofk, lambda: call((-1, 2)), f"{entry}: counts[0]=-1 outside 0..4")
    call((4, 0))


# ---------------------------------------------------------------------------------------------------- the three downloads
def frames():
    rng = np.random.default_rng(11)
    blocks = rng.integers(0, 256, (B, H // 4 + 1, W // 4 + 1)).astype(np.uint8)
    big = np.kron(blocks, np.ones((4, 4), np.uint8))
    prev, nxt = big[:, 1:H + 1, 1:W + 1], big[:, 1:H + 1, 0:W]   # one pixel to the right
    return np.repeat(prev[..., None], 3, -1).copy(), np.repeat(nxt[..., None], 3, -1).copy()


def run_settings(ofk):
    """name -> (setter name, struct for the run, download entry, the stage entry on the downloaded raw points)."""
    cam = ofk.camera_setting("brown", fx=60.0, cx=W / 2.0, cy=H / 2.0, k=(-0.1, 0.02))
    rs = ofk.rshutter_setting("gyro", readout=0.9, anchor=0.5)
    rs_stage = ofk.RShutter(rs.mode, H, rs.readout, rs.anchor, rs.omega_gain)
    fm = ofk.finite_motion_setting()
    return {
        "camera": ("set_camera", cam, "ofk_camera_download", "ofk_set_camera",
                   lambda c, o, sn: (c.undistort_points(cam, o["prev_pts"], o["counts"]), c.undistort_points(cam, o["next_pts"], o["counts"]))),
        "rolling_shutter": ("set_rolling_shutter", rs, "ofk_rs_download", "ofk_set_rolling_shutter",
                            lambda c, o, sn: c.rs_correct_points(rs_stage, o["prev_pts"], o["next_pts"], o["counts"], sensors=sn)),
        "finite_motion": ("set_finite_motion", fm, "ofk_finite_download", "ofk_set_finite_motion",
                          lambda c, o, sn: c.finite_correct_points(fm, o["prev_pts"], o["next_pts"], o["counts"], sensors=sn)),
    }


@pytest.mark.parametrize("name", ["camera", "rolling_shutter", "finite_motion"])
def test_point_download_before_and_after_a_run(ofk, name):
    setter, struct, entry, _, stage = run_settings(ofk)[name]
    methods = dict(camera=ofk.Context.camera_download, rolling_shutter=ofk.Context.rs_download, finite_motion=ofk.Context.finite_download)
    downloads = {n: (methods[n], v[2], v[3]) for n, v in run_settings(ofk).items()}
    params = ofk.Params(PTS, 0.01, 3.0, 3, 9, 1, 20, 0.03, 1e-4, ofk.SOLVE_NODE, 0, 0.0)
    sensors = sensors_of(ofk)
    prev, nxt = frames()
    c = ofk.Context(0, W, H, B, PTS, 1)
    try:
        c.pairs_upload(prev, nxt); c.pairs_set_sensors(sensors)
        c.pairs_run(params)                                      # a run with the setting off is no run with it on
        getattr(c, setter)(struct)
        for n, (method, e, s) in downloads.items():
            refused(ofk, lambda: method(c, B), f"{e}: no run or step with {s} on yet")
        c.pairs_run(params)
        out = c.pairs_download()
        for n, (method, e, s) in downloads.items():              # the other two settings have had no run
            if n != name:
                refused(ofk, lambda: method(c, B), f"{e}: no run or step with {s} on yet")
        assert out["counts"].min() >= 6, out["counts"]
        fn = getattr(c._L, entry)
        full = [np.full((B, PTS, 2), SENTINEL), np.full((B, PTS, 2), SENTINEL)]
        assert fn(c._h, ofk._p(full[0]), ofk._p(full[1]), PTS) == 0
        ref = stage(c, out, sensors)
        moved = 0.0
        for b in range(B):
            n = int(out["counts"][b])
            for k in range(2):
                assert np.array_equal(bits(full[k][b, :n]), bits(ref[k][b, :n])), (name, b, k)
            moved = max(moved, float(np.abs(full[1][b, :n] - out["next_pts"][b, :n]).max()))
        assert moved > 1e-3, moved                               # the correction is not the identity here
        m = downloads[name][0](c, B)
        assert np.array_equal(bits(m[0]), bits(full[0])) and np.array_equal(bits(m[1]), bits(full[1]))
        assert downloads[name][0](c, 1)[0].shape == (1, PTS, 2)
        for stride in (5, PTS, 40):
            n = min(stride, PTS)
            got = [np.full((B, stride, 2), SENTINEL), np.full((B, stride, 2), SENTINEL)]
            assert fn(c._h, ofk._p(got[0]), ofk._p(got[1]), stride) == 0
            for k in range(2):
                assert np.array_equal(bits(got[k][:, :n]), bits(full[k][:, :n])), (name, stride, k)
                assert np.all(got[k][:, n:] == SENTINEL), (name, stride, k)
            for k in range(2):                                   # one NULL pointer: the other array alone
                one = np.full((B, stride, 2), SENTINEL)
                assert fn(c._h, *((ofk._p(one), None) if k == 0 else (None, ofk._p(one))), stride) == 0
                assert np.array_equal(bits(one), bits(got[k])), (name, stride, k)
        assert fn(c._h, None, None, 0) == ofk.E_INVALID
        assert c._L.ofk_last_error(c._h).decode() == f"{entry}: stride 0"
    finally:
        c.close()
