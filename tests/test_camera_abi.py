"""The camera-model entry points exist in the header, the binding and the library; the setting's structure agrees on both sides; the
kernels are in the code object; camera_setting's defaults and every invalid field; the pipeline configuration and optical_fusion carry
the setting; cv2_hip's argument rules (CPU-only).  On a device: the setting's default, its round trip, every invalid field, "off"
after NULL, and the download's refusal before a run."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_camera", "ofk_get_camera", "ofk_undistort_points", "ofk_distort_points", "ofk_camera_download")
FIELDS = ["model", "iters", "fx", "fy", "cx", "cy", "k", "fo_x", "fo_y", "co_x", "co_y"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge


def values(m):
    return [list(m.k) if n == "k" else getattr(m, n) for n in FIELDS]


def test_entry_points_declared_bound_and_exported(built, ofk):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofk.h")).read(), flags=re.S)
    lib = ofk.load_library()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert s in ofk.SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
    for name, val in (("OFK_CAMERA_OFF", 0), ("OFK_CAMERA_BROWN", 1), ("OFK_CAMERA_FISHEYE", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
    assert (ofk.CAMERA_OFF, ofk.CAMERA_BROWN, ofk.CAMERA_FISHEYE) == (0, 1, 2)
    assert ofk.CAMERA_MODELS == {"off": 0, "brown": 1, "fisheye": 2}
    m = re.search(r"typedef struct ofk_camera \{(.*?)\} ofk_camera;", txt, flags=re.S)
    assert m and [n for _, n in re.findall(r"\b(int|double)\s+(\w+)(?:\[8\])?;", m.group(1))] == FIELDS
    assert re.search(r"double\s+k\[8\];", m.group(1))
    assert [n for n, _ in ofk.Camera._fields_] == FIELDS
    assert [t for _, t in ofk.Camera._fields_] == [C.c_int] * 2 + [C.c_double] * 4 + [C.c_double * 8] + [C.c_double] * 4
    assert C.sizeof(ofk.Camera) == 8 + 16 * 8 and ofk.Camera.fx.offset == 8 and ofk.Camera.k.offset == 40 and ofk.Camera.fo_x.offset == 104
    assert len(lib.ofk_undistort_points.argtypes) == 7 and len(lib.ofk_distort_points.argtypes) == 7 and len(lib.ofk_camera_download.argtypes) == 4
    assert lib.ofk_set_camera(None, None) == ofk.E_INVALID and lib.ofk_get_camera(None, None) == ofk.E_INVALID
    cam = ofk.camera_setting(fx=100.0)
    assert lib.ofk_undistort_points(None, C.byref(cam), None, None, 1, 1, None) == ofk.E_INVALID
    assert lib.ofk_distort_points(None, C.byref(cam), None, None, 1, 1, None) == ofk.E_INVALID
    assert lib.ofk_camera_download(None, None, None, 1) == ofk.E_INVALID


def test_camera_kernels_are_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for k in (b"k_camera_undistortILi1E", b"k_camera_undistortILi2E", b"k_camera_distortILi1E", b"k_camera_distortILi2E", b"k_seed_points"):
        assert k in blob, k


def test_settings_from_names(built, ofk):
    m = ofk.camera_setting(fx=1000.0)
    assert values(m) == [1, 20, 1000.0, 1000.0, 0.0, 0.0, [0.0] * 8, 1000.0, 1000.0, 0.0, 0.0]
    m = ofk.camera_setting("fisheye", 1000.0, 1010.0, 652.3, 470.1, (-0.03, 0.005, -0.001, 0.0002))
    assert values(m) == [2, 10, 1000.0, 1010.0, 652.3, 470.1, [-0.03, 0.005, -0.001, 0.0002, 0, 0, 0, 0], 1000.0, 1000.0, 652.3, 470.1]
    m = ofk.camera_setting("brown", 900.0, 910.0, 1.0, 2.0, (1, 2, 3, 4, 5, 6, 7, 8), iters=50, fo_x=3.0, fo_y=4.0, co_x=5.0, co_y=6.0)
    assert values(m) == [1, 50, 900.0, 910.0, 1.0, 2.0, [1, 2, 3, 4, 5, 6, 7, 8], 3.0, 4.0, 5.0, 6.0]
    assert ofk.camera_setting(ofk.CAMERA_FISHEYE, fx=2.0, iters=1).iters == 1
    assert ofk.camera_setting("off", fx=0.0, iters=0).model == 0               # off: the other fields are not looked at
    nan, inf = float("nan"), float("inf")
    for bad in (dict(model="pinhole"), dict(model=3), dict(model=-1), dict(iters=0), dict(iters=51), dict(fx=0.0), dict(fy=0.0), dict(fo_x=0.0),
                dict(fo_y=0.0), dict(fx=nan), dict(fy=inf), dict(cx=nan), dict(cy=-inf), dict(k=(nan,)), dict(k=(0, 0, 0, inf)), dict(fo_x=nan),
                dict(fo_y=inf), dict(co_x=nan), dict(co_y=inf), dict(k=(0,) * 9), dict(model="fisheye", k=(0, 0, 0, 0, 0.1)),
                dict(model="fisheye", k=(0, 0, 0, 0, 0, 0, 0, 1e-9))):
        with pytest.raises(ValueError):
            ofk.camera_setting(**dict(dict(fx=100.0), **bad))
    with pytest.raises(TypeError):
        ofk.camera_setting(fx=1.0, skew=0.1)


class Recorder:
    """Stands in for ofk.Context: records what a pipeline applies to it."""
    calls = []

    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        def f(*a, **k):
            Recorder.calls.append((name, a, k))
        return f


def test_pipeline_config_carries_the_setting(built, pkg, ofk, monkeypatch):
    from of_amd import pipeline
    from of_amd.pipeline import CameraModel, PipelineConfig, FlowPipeline, FlowStream
    for cfg in (PipelineConfig(), PipelineConfig.node(), PipelineConfig.of_module(), PipelineConfig.evaluate_exp(), PipelineConfig.baseline_1080p()):
        assert cfg.camera is None and cfg.camera_setting() is None
    cm = CameraModel(fx=1000.0, fy=1010.0, cx=652.3, cy=470.1, k=(-0.28, 0.09, 0.0008, -0.0005, -0.012))
    assert cm.sensor_slots() == (1.0 / 1000.0, 652.3, 470.1)
    assert CameraModel(fx=1000.0, fo=800.0, co_x=1.0, co_y=2.0).sensor_slots() == (1.0 / 800.0, 1.0, 2.0)
    assert values(cm.setting()) == [1, 20, 1000.0, 1010.0, 652.3, 470.1, [-0.28, 0.09, 0.0008, -0.0005, -0.012, 0, 0, 0], 1000.0, 1000.0, 652.3, 470.1]
    assert CameraModel(fx=5.0, model="fisheye").setting().iters == 10 and CameraModel(fx=5.0, iters=7).setting().iters == 7
    on = PipelineConfig(camera=cm)
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params())          # to_params() does not know the setting
    assert PipelineConfig(camera=CameraModel(fx=1.0, model="off")).camera_setting() is None
    with pytest.raises(ValueError):
        PipelineConfig(camera=CameraModel(fx=0.0)).camera_setting()
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    Recorder.calls = []
    s = FlowStream(64, 48, batch=1, cfg=PipelineConfig())
    p = FlowPipeline(64, 48, batch=1, cfg=PipelineConfig())
    assert not [c for c in Recorder.calls if c[0] == "set_camera"] and callable(s.ideal_points) and callable(p.ideal_points)
    FlowStream(64, 48, batch=1, cfg=on)
    FlowPipeline(64, 48, batch=1, cfg=on)
    sets = [c for c in Recorder.calls if c[0] == "set_camera"]
    assert len(sets) == 2 and all(values(c[1][0]) == values(cm.setting()) for c in sets)


def test_optical_fusion_hands_the_camera_to_its_pipeline_config(built, pkg, ofk):
    from of_amd.pipeline import CameraModel, PipelineConfig
    from of_amd.velocity_node import optical_fusion
    assert optical_fusion(spin=False)._camera == {}
    node = optical_fusion(spin=False, camera=dict(fx=1000.0, fy=1010.0, cx=652.3, cy=470.1, k=(-0.28, 0.09, 0, 0)))
    cm = node._camera["camera"]
    assert isinstance(cm, CameraModel) and cm.sensor_slots() == (1e-3, 652.3, 470.1)
    assert values(PipelineConfig(**node._camera).camera_setting())[:6] == [1, 20, 1000.0, 1010.0, 652.3, 470.1]
    given = CameraModel(fx=3.0, model="fisheye")
    assert optical_fusion(spin=False, camera=given)._camera["camera"] is given
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, camera=dict(fx=0.0))
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, camera=dict(fx=1.0, skew=3))


def test_cv2_argument_rules(built, pkg, ofk):
    """What cv2_hip refuses before it needs a device."""
    from of_amd import cv2_hip as cv2
    K = np.array([[1000.0, 0, 652.3], [0, 1010.0, 470.1], [0, 0, 1]])
    p32 = np.zeros((3, 1, 2), np.float32)
    with pytest.raises(ValueError):
        cv2.undistortPoints(p32.astype(np.float64), K, np.zeros(5))
    with pytest.raises(NotImplementedError):
        cv2.undistortPoints(p32, K, np.zeros(5), R=np.diag([1.0, 1.0, -1.0]))
    with pytest.raises(ValueError):
        cv2.undistortPoints(p32, K, np.zeros(6))
    with pytest.raises(ValueError):
        cv2.fisheye.undistortPoints(p32, K, np.zeros(5))
    with pytest.raises(NotImplementedError):
        cv2.fisheye.distortPoints(p32, K, np.zeros(4), alpha=0.1)
    with pytest.raises(NotImplementedError):
        cv2.fisheye.undistortPoints(p32, K, np.zeros(4), R=np.zeros((3, 3)))
    empty = cv2.undistortPoints(np.zeros((0, 1, 2), np.float32), K, np.zeros(4), R=np.eye(3))
    assert empty.shape == (0, 1, 2)


@pytest.mark.gpu
def test_setting_round_trip_invalid_fields_and_off_after_null(pkg, ofk):
    ctx = ofk.Context(0, 64, 48, 2, 100, 2)
    try:
        assert values(ctx.get_camera()) == [0, 20, 1.0, 1.0, 0.0, 0.0, [0.0] * 8, 1.0, 1.0, 0.0, 0.0]          # off
        with pytest.raises(ofk.OfkError) as e:                     # no run with the setting on yet
            ctx.camera_download(1)
        assert e.value.code == ofk.E_INVALID
        good = dict(model=1, iters=30, fx=1000.0, fy=1010.0, cx=652.3, cy=470.1, k=(-0.28, 0.09, 0.0008, -0.0005, -0.012, 0.1, 0.2, 0.3),
                    fo_x=900.0, fo_y=900.0, co_x=640.0, co_y=480.0)

        def make(**over):
            d = dict(good, **over)
            return ofk.Camera(d["model"], d["iters"], d["fx"], d["fy"], d["cx"], d["cy"], (C.c_double * 8)(*(list(d["k"]) + [0.0] * (8 - len(d["k"])))),
                              d["fo_x"], d["fo_y"], d["co_x"], d["co_y"])
        ctx.set_camera(make())
        assert values(ctx.get_camera()) == values(make())
        nan, inf = float("nan"), float("inf")
        pts = np.zeros((1, 4, 2), np.float32)
        for bad in (dict(model=3), dict(model=-1), dict(iters=0), dict(iters=51), dict(fx=0.0), dict(fy=0.0), dict(fo_x=0.0, fo_y=0.0), dict(fx=nan),
                    dict(fy=inf), dict(cx=nan), dict(cy=-inf), dict(k=(nan,)), dict(k=(0, 0, 0, 0, 0, 0, 0, inf)), dict(fo_x=nan, fo_y=nan),
                    dict(co_x=nan), dict(co_y=inf), dict(model=2), dict(model=2, k=(0, 0, 0, 0, 0, 0, 0, 1e-9))):
            for call in (ctx.set_camera, lambda m: ctx.undistort_points(m, pts), lambda m: ctx.distort_points(m, pts)):
                with pytest.raises(ofk.OfkError) as e:
                    call(make(**bad))
                assert e.value.code == ofk.E_INVALID, bad
            assert values(ctx.get_camera()) == values(make()), bad                     # the previous setting is in place
        with pytest.raises(ofk.OfkError):                          # one scaling in the solve: the setting needs one focal length
            ctx.set_camera(make(fo_y=901.0))
        assert ctx.undistort_points(make(fo_y=901.0), pts).shape == (1, 4, 2)         # the stage entries take two
        with pytest.raises(ofk.OfkError):                          # off is no model for a stage entry
            ctx.undistort_points(make(model=0), pts)
        ctx.set_camera(None)
        assert ctx.get_camera().model == 0 and ctx.get_camera().iters == 30
        ctx.set_camera(fx=5.0)
        ctx.set_camera(ofk.Camera(0, -9, nan, 0.0, 0.0, 0.0, (C.c_double * 8)(), 0.0, 0.0, 0.0, 0.0))       # model off: off, whatever else it holds
        assert ctx.get_camera().model == 0 and ctx.get_camera().fx == 5.0
    finally:
        ctx.close()
