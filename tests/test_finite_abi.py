"""The finite-motion entry points exist in the header, the binding and the library; the setting's structure agrees on both sides; the
kernel is in the code object; finite_motion_setting's defaults and every invalid field; the pipeline configuration and optical_fusion
carry the setting (CPU-only).  On a device: the setting's default, its round trip, every refusal leaving the setting as it was, "off"
after NULL, and the download's refusal before a run."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_finite_motion", "ofk_get_finite_motion", "ofk_finite_correct_points", "ofk_finite_download")
FIELDS = ["mode", "min_depth"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge


def values(m):
    return [getattr(m, n) for n in FIELDS]


def test_entry_points_declared_bound_and_exported(built, ofk):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofk.h")).read(), flags=re.S)
    lib = ofk.load_library()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert s in ofk.SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
    for name, val in (("OFK_FM_OFF", 0), ("OFK_FM_EXACT", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
    assert (ofk.FM_OFF, ofk.FM_EXACT) == (0, 1)
    assert ofk.FM_MODES == {"off": 0, "exact": 1}
    m = re.search(r"typedef struct ofk_finite_motion \{(.*?)\} ofk_finite_motion;", txt, flags=re.S)
    assert m and [n for _, n in re.findall(r"\b(int|double)\s+(\w+);", m.group(1))] == FIELDS
    assert [n for n, _ in ofk.FiniteMotion._fields_] == FIELDS
    assert [t for _, t in ofk.FiniteMotion._fields_] == [C.c_int, C.c_double]
    assert C.sizeof(ofk.FiniteMotion) == 16 and ofk.FiniteMotion.min_depth.offset == 8
    assert len(lib.ofk_finite_correct_points.argtypes) == 10 and len(lib.ofk_finite_download.argtypes) == 4
    assert lib.ofk_set_finite_motion(None, None) == ofk.E_INVALID and lib.ofk_get_finite_motion(None, None) == ofk.E_INVALID
    fm = ofk.finite_motion_setting()
    assert lib.ofk_finite_correct_points(None, C.byref(fm), None, None, None, 1, 1, None, None, None) == ofk.E_INVALID
    assert lib.ofk_finite_download(None, None, None, 1) == ofk.E_INVALID


def test_finite_kernel_is_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for k in (b"k_finite_correct", b"k_rs_correctILi2E", b"k_camera_undistortILi1E"):
        assert k in blob, k


def test_settings_from_names(built, ofk):
    assert values(ofk.finite_motion_setting()) == [1, 0.1]
    assert values(ofk.finite_motion_setting("exact", 1.0)) == [1, 1.0]
    assert values(ofk.finite_motion_setting(ofk.FM_EXACT, 1e-6)) == [1, 1e-6]
    assert ofk.finite_motion_setting("off", min_depth=-3.0).mode == 0            # off: the other field is not looked at
    nan, inf = float("nan"), float("inf")
    for bad in (dict(mode="linear"), dict(mode=2), dict(mode=-1), dict(min_depth=0.0), dict(min_depth=-0.1), dict(min_depth=1.0000001),
                dict(min_depth=nan), dict(min_depth=inf), dict(min_depth=-inf)):
        with pytest.raises(ValueError):
            ofk.finite_motion_setting(**bad)
    with pytest.raises(TypeError):
        ofk.finite_motion_setting(max_depth=0.1)


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
    from of_amd.pipeline import PipelineConfig, FlowPipeline, FlowStream
    for cfg in (PipelineConfig(), PipelineConfig.node(), PipelineConfig.of_module(), PipelineConfig.evaluate_exp(), PipelineConfig.baseline_1080p()):
        assert cfg.finite_motion is None and cfg.finite_motion_setting() is None
    assert values(PipelineConfig(finite_motion=True).finite_motion_setting()) == [1, 0.1]
    given = ofk.finite_motion_setting(min_depth=0.25)
    on = PipelineConfig(finite_motion=given)
    assert values(on.finite_motion_setting()) == [1, 0.25]
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params())          # to_params() does not know the setting
    assert PipelineConfig(finite_motion=ofk.finite_motion_setting("off")).finite_motion_setting() is None
    assert PipelineConfig(finite_motion=False).finite_motion_setting() is None
    with pytest.raises(ValueError):
        PipelineConfig(finite_motion=ofk.FiniteMotion(1, 2.0)).finite_motion_setting()
    with pytest.raises(ValueError):
        PipelineConfig(finite_motion=ofk.FiniteMotion(7, 0.1)).finite_motion_setting()
    with pytest.raises(ValueError):
        PipelineConfig(finite_motion="exact").finite_motion_setting()
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    Recorder.calls = []
    s = FlowStream(64, 48, batch=1, cfg=PipelineConfig())
    p = FlowPipeline(64, 48, batch=1, cfg=PipelineConfig())
    assert not [c for c in Recorder.calls if c[0] == "set_finite_motion"] and callable(s.ideal_points) and callable(p.ideal_points)
    FlowStream(64, 48, batch=1, cfg=on)
    FlowPipeline(64, 48, batch=1, cfg=on)
    sets = [c for c in Recorder.calls if c[0] == "set_finite_motion"]
    assert len(sets) == 2 and all(values(c[1][0]) == [1, 0.25] for c in sets)


def test_optical_fusion_hands_the_setting_to_its_pipeline_config(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    from of_amd import velocity_node
    from of_amd.velocity_node import optical_fusion
    assert callable(velocity_node.finite_points)
    assert optical_fusion(spin=False)._finite_motion == {}
    assert optical_fusion(spin=False, finite_motion=False)._finite_motion == {}
    node = optical_fusion(spin=False, finite_motion=True)
    assert values(PipelineConfig(**node._finite_motion).finite_motion_setting()) == [1, 0.1]
    node = optical_fusion(spin=False, finite_motion=dict(min_depth=0.5))
    assert values(PipelineConfig(**node._finite_motion).finite_motion_setting()) == [1, 0.5]
    given = ofk.finite_motion_setting(min_depth=0.2)
    assert optical_fusion(spin=False, finite_motion=given)._finite_motion["finite_motion"] is given
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, finite_motion=dict(min_depth=2.0))
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, finite_motion=dict(max_depth=3))


@pytest.mark.gpu
def test_setting_round_trip_every_refusal_and_off_after_null(pkg, ofk):
    ctx = ofk.Context(0, 64, 48, 2, 100, 2)
    try:
        assert values(ctx.get_finite_motion()) == [0, 0.1]         # off
        with pytest.raises(ofk.OfkError) as e:                     # no run with the setting on yet
            ctx.finite_download(1)
        assert e.value.code == ofk.E_INVALID
        good = ofk.FiniteMotion(1, 0.25)
        ctx.set_finite_motion(good)
        assert values(ctx.get_finite_motion()) == [1, 0.25]
        nan, inf = float("nan"), float("inf")
        pts = np.zeros((1, 4, 2), np.float32)
        sn = ofk.make_sensors(1)
        for bad in ((2, 0.25), (-1, 0.25), (1, 0.0), (1, -0.5), (1, 1.0000001), (1, nan), (1, inf), (1, -inf)):
            for call in (ctx.set_finite_motion, lambda m: ctx.finite_correct_points(m, pts, pts, sensors=sn)):
                with pytest.raises(ofk.OfkError) as e:
                    call(ofk.FiniteMotion(*bad))
                assert e.value.code == ofk.E_INVALID, bad
            assert values(ctx.get_finite_motion()) == [1, 0.25], bad                     # the previous setting is in place
        with pytest.raises(ofk.OfkError) as e:                     # the stage entry needs the sensors
            ctx.finite_correct_points(good, pts, pts)
        assert e.value.code == ofk.E_INVALID
        with pytest.raises(ofk.OfkError):                          # off is no mode for a stage entry
            ctx.finite_correct_points(ofk.FiniteMotion(0, 0.25), pts, pts, sensors=sn)
        assert ctx.finite_correct_points(ofk.FiniteMotion(1, 1.0), pts, pts, sensors=sn)[0].shape == (1, 4, 2)
        assert values(ctx.get_finite_motion()) == [1, 0.25]        # the stage entry touches no setting
        ctx.set_finite_motion(ofk.FiniteMotion(1, 1.0))            # the closed end of the range is inside
        ctx.set_finite_motion(None)
        assert values(ctx.get_finite_motion()) == [0, 1.0]
        ctx.set_finite_motion(min_depth=0.5)
        ctx.set_finite_motion(ofk.FiniteMotion(0, nan))            # mode off: off, whatever else it holds
        assert values(ctx.get_finite_motion()) == [0, 0.5]
        with pytest.raises(ofk.OfkError):
            ctx.finite_download(1)
    finally:
        ctx.close()
