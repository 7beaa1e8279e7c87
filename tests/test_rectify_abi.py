"""The warp through a lens and the rectify setting exist in the header, the binding and the library; defaults mean off; the
configuration accepts a camera beside the stabilised view exactly when rectify is on; the facade refuses what is out of scope before
it asks for a device (CPU-only)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_warp_lens", "ofk_set_rectify", "ofk_get_rectify")
LENS = dict(fx=160.0, fy=160.0, cx=80.0, cy=64.0, k=(-0.1, 0.01, 0, 0))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge


def test_entry_points_declared_bound_and_exported(built, ofk):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofk.h")).read(), flags=re.S)
    lib = ofk.load_library()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert s in ofk.SYMBOLS and hasattr(lib, s) and getattr(lib, s).argtypes is not None, s
    m = re.search(r"int ofk_warp_lens\s*\((.*?)\);", txt, flags=re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == \
        "ofk_ctx *ctx, const struct ofk_camera *cam, const uint8_t *src, int sh, int sw, int channels, const double *M, uint8_t *dst, " \
        "int dh, int dw, int border, int border_value, double r_max, int batch, int *covered"
    assert len(lib.ofk_warp_lens.argtypes) == 15
    for name, val in (("OFK_RECTIFY_OFF", 0), ("OFK_RECTIFY_ON", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
        assert getattr(ofk, name[4:]) == val, name
    m = re.search(r"typedef struct ofk_rectify \{(.*?)\} ofk_rectify;", txt, flags=re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "int mode; double r_max;"
    assert list(ofk.Rectify._fields_) == [("mode", C.c_int), ("r_max", C.c_double)] and C.sizeof(ofk.Rectify) == 16
    assert ("rectify", ofk.Rectify) in ofk.SETTINGS
    assert lib.ofk_set_rectify(None, None) == ofk.E_INVALID and lib.ofk_get_rectify(None, None) == ofk.E_INVALID
    assert lib.ofk_warp_lens(None, None, None, 1, 1, 1, None, None, 1, 1, 0, 0, 0.0, 1, None) == ofk.E_INVALID
    assert callable(ofk.Context.warp_lens) and callable(ofk.Context.set_rectify) and callable(ofk.Context.get_rectify)


def test_lens_kernels_are_in_the_code_object(built, ofk):
    """Both channel counts, the two Brown forms (with and without the rational terms' divide) and the fisheye."""
    blob = open(ofk.LIB_PATH, "rb").read()
    for ch in (1, 3):
        for tail in (b"Li1ELb1E", b"Li1ELb0E", b"Li2ELb1E"):
            assert b"k_warp_lens_u8ILi%dE" % ch + tail in blob, (ch, tail)


def test_settings_from_names(built, ofk):
    assert (ofk.rectify_setting().mode, ofk.rectify_setting().r_max) == (1, 0.0)
    r = ofk.rectify_setting(True, 1.25)
    assert (r.mode, r.r_max) == (ofk.RECTIFY_ON, 1.25)
    assert ofk.rectify_setting(False, r_max=-3.0).mode == 0        # off: the other field is not looked at
    for bad in (dict(mode=2), dict(mode=-1), dict(r_max=float("nan")), dict(r_max=float("inf")), dict(r_max=-0.5)):
        with pytest.raises(ValueError):
            ofk.rectify_setting(**bad)
    with pytest.raises(TypeError):
        ofk.rectify_setting(radius=3)


class Recorder:
    """Stands in for ofk.Context: records what a pipeline applies to it."""
    calls = []

    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        def f(*a, **k):
            Recorder.calls.append((name, a, k))
        return f


def test_pipeline_config_default_means_off_and_rectify_admits_the_camera(built, pkg, ofk, monkeypatch):
    from of_amd import pipeline
    from of_amd.pipeline import CameraModel, FlowStream, PipelineConfig, RollingShutter
    cam = CameraModel(**LENS)
    for cfg in (PipelineConfig(), PipelineConfig.node(), PipelineConfig.baseline_1080p(), PipelineConfig(track_table=True, keyframe=True, stabilise=True)):
        assert cfg.rectify is None and cfg.rectify_setting() is None
    assert PipelineConfig(rectify=False).rectify_setting() is None and PipelineConfig(rectify=ofk.rectify_setting(False)).rectify_setting() is None
    base = dict(track_table=True, keyframe=True, stabilise=True)
    with pytest.raises(ValueError):                                # as before: a camera without rectify
        PipelineConfig(**base, camera=cam).stabilise_setting()
    with pytest.raises(ValueError):
        PipelineConfig(**base, camera=cam, rectify=False).stabilise_setting()
    on = PipelineConfig(**base, camera=cam, rectify=ofk.rectify_setting(r_max=1.5))
    assert on.stabilise_setting().mode == ofk.STAB_PLANE and (on.rectify_setting().mode, on.rectify_setting().r_max) == (1, 1.5)
    assert PipelineConfig(**base, camera=cam, rectify=True).rectify_setting().r_max == 0.0
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params())
    assert PipelineConfig(**base, rectify=True).stabilise_setting() is not None       # inert without a camera
    for rs in (dict(), dict(camera=cam)):                         # the rolling shutter stays refused either way
        with pytest.raises(ValueError):
            PipelineConfig(**base, **rs, rectify=True, rolling_shutter=RollingShutter(mode="flow", readout=0.5)).stabilise_setting()
    for bad in ("on", ofk.Rectify(1, -1.0), ofk.Rectify(1, float("nan")), ofk.Rectify(1, float("inf")), ofk.Rectify(2, 0.0)):
        with pytest.raises(ValueError):
            PipelineConfig(rectify=bad).rectify_setting()
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    Recorder.calls = []
    FlowStream(64, 48, batch=1, cfg=PipelineConfig(**base))
    assert not [c for c in Recorder.calls if c[0] == "set_rectify"]
    Recorder.calls = []
    FlowStream(64, 48, batch=1, cfg=on)
    names = [c[0] for c in Recorder.calls]
    sets = [c for c in Recorder.calls if c[0] == "set_rectify"]
    assert len(sets) == 1 and (sets[0][1][0].mode, sets[0][1][0].r_max) == (1, 1.5)
    assert names.index("set_rectify") < names.index("set_stabilise") and "set_camera" in names
    Recorder.calls = []                                            # independent pairs have no view: FlowPipeline ignores the setting
    pipeline.FlowPipeline(64, 48, batch=1, cfg=on)
    assert not [c for c in Recorder.calls if c[0] in ("set_rectify", "set_stabilise")]


def test_optical_fusion_hands_the_setting_down(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig, RollingShutter
    from of_amd import velocity_node
    from of_amd.velocity_node import optical_fusion
    assert optical_fusion(spin=False, stabilise=True)._rectify == {}
    with pytest.raises((TypeError, ValueError)):                   # as before
        optical_fusion(spin=False, stabilise=True, camera=dict(LENS))
    node = optical_fusion(spin=False, stabilise=True, camera=dict(LENS), rectify=dict(r_max=1.2))
    cfg = PipelineConfig(**node._track_table, **node._keyframe, **node._stabilise, **node._camera, **node._rectify)
    assert cfg.stabilise_setting() is not None and cfg.rectify_setting().r_max == 1.2
    assert optical_fusion(spin=False, stabilise=True, camera=dict(LENS), rectify=True)._rectify == dict(rectify=True)
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, stabilise=True, camera=dict(LENS), rectify=dict(r_max=-1.0))
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, stabilise=True, rectify=True, rolling_shutter=RollingShutter(mode="flow", readout=0.5))
    assert callable(velocity_node.rectify_frame)


def test_facade_refuses_skew_and_other_interpolations_before_any_device(built, pkg):
    from of_amd import cv2_hip
    img = np.zeros((8, 8), np.uint8)
    K = np.array([[10.0, 0, 4], [0, 10.0, 4], [0, 0, 1]])
    skew = K.copy(); skew[0, 1] = 0.01
    with pytest.raises(NotImplementedError):
        cv2_hip.undistort(img, skew, np.zeros(5))
    with pytest.raises(NotImplementedError):
        cv2_hip.undistort(img, K, np.zeros(5), newCameraMatrix=skew)
    with pytest.raises(NotImplementedError):
        cv2_hip.fisheye.undistortImage(img, skew, np.zeros(4))
    with pytest.raises(NotImplementedError):
        cv2_hip.fisheye.undistortImage(img, K, np.zeros(4), Knew=skew)
    for flags in (cv2_hip.INTER_NEAREST, cv2_hip.INTER_CUBIC, cv2_hip.INTER_AREA, cv2_hip.INTER_LANCZOS4):
        with pytest.raises(NotImplementedError):
            cv2_hip.undistort(img, K, np.zeros(5), flags=flags)
        with pytest.raises(NotImplementedError):
            cv2_hip.fisheye.undistortImage(img, K, np.zeros(4), flags=flags)
    with pytest.raises(ValueError):
        cv2_hip.undistort(img, K, np.zeros(3))
    with pytest.raises(ValueError):
        cv2_hip.fisheye.undistortImage(img, K, np.zeros(5))
    for bad in (np.zeros((8, 8), np.float32), np.zeros((8, 8, 2), np.uint8)):
        with pytest.raises(ValueError):
            cv2_hip.undistort(bad, K, np.zeros(5))
    for dst in (np.zeros((8, 9), np.uint8), np.zeros((8, 8), np.float32), [[0] * 8] * 8):      # a dst that cannot be filled is refused
        with pytest.raises(ValueError):
            cv2_hip.undistort(img, K, np.zeros(5), dst)
