"""The rolling-shutter entry points exist in the header, the binding and the library; the setting's structure agrees on both sides; the
kernels are in the code object; rshutter_setting's defaults and every invalid field; the pipeline configuration and optical_fusion
carry the setting (CPU-only).  On a device: the setting's default, its round trip, every refusal leaving the setting as it was, "off"
after NULL, and the download's refusal before a run."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_rolling_shutter", "ofk_get_rolling_shutter", "ofk_rs_correct_points", "ofk_rs_download")
FIELDS = ["mode", "rows", "readout", "anchor", "omega_gain"]


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
    for name, val in (("OFK_RS_OFF", 0), ("OFK_RS_FLOW", 1), ("OFK_RS_GYRO", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
    assert (ofk.RS_OFF, ofk.RS_FLOW, ofk.RS_GYRO) == (0, 1, 2)
    assert ofk.RS_MODES == {"off": 0, "flow": 1, "gyro": 2}
    m = re.search(r"typedef struct ofk_rshutter \{(.*?)\} ofk_rshutter;", txt, flags=re.S)
    assert m and [n for _, n in re.findall(r"\b(int|double)\s+(\w+);", m.group(1))] == FIELDS
    assert [n for n, _ in ofk.RShutter._fields_] == FIELDS
    assert [t for _, t in ofk.RShutter._fields_] == [C.c_int] * 2 + [C.c_double] * 3
    assert C.sizeof(ofk.RShutter) == 32 and ofk.RShutter.readout.offset == 8 and ofk.RShutter.omega_gain.offset == 24
    assert len(lib.ofk_rs_correct_points.argtypes) == 12 and len(lib.ofk_rs_download.argtypes) == 4
    assert lib.ofk_set_rolling_shutter(None, None) == ofk.E_INVALID and lib.ofk_get_rolling_shutter(None, None) == ofk.E_INVALID
    rs = ofk.rshutter_setting("flow", 0.5, rows=100)
    assert lib.ofk_rs_correct_points(None, C.byref(rs), None, None, None, None, None, 1, 1, None, None, None) == ofk.E_INVALID
    assert lib.ofk_rs_download(None, None, None, 1) == ofk.E_INVALID


def test_rs_kernels_are_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for k in (b"k_rs_correctILi1E", b"k_rs_correctILi2E", b"k_camera_undistortILi1E", b"k_seed_points"):
        assert k in blob, k


def test_settings_from_names(built, ofk):
    assert values(ofk.rshutter_setting(readout=0.9)) == [2, 0, 0.9, 0.5, 1.0]
    assert values(ofk.rshutter_setting("flow", -0.5, 0.0, 960, 2.0)) == [1, 960, -0.5, 0.0, 2.0]
    assert values(ofk.rshutter_setting(ofk.RS_GYRO, 1.0, 1.0, None, -1.0)) == [2, 0, 1.0, 1.0, -1.0]
    assert ofk.rshutter_setting("off", readout=7.0, anchor=-3.0, omega_gain=0.0).mode == 0          # off: the other fields are not looked at
    nan, inf = float("nan"), float("inf")
    for bad in (dict(mode="global"), dict(mode=3), dict(mode=-1), dict(readout=1.0000001), dict(readout=-1.5), dict(readout=nan), dict(readout=inf),
                dict(anchor=-1e-9), dict(anchor=1.0000001), dict(anchor=nan), dict(rows=-1), dict(rows=65537), dict(omega_gain=0.0), dict(omega_gain=nan),
                dict(omega_gain=-inf)):
        with pytest.raises(ValueError):
            ofk.rshutter_setting(**dict(dict(readout=0.5), **bad))
    with pytest.raises(TypeError):
        ofk.rshutter_setting(readout=0.5, exposure=0.1)


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
    from of_amd.pipeline import PipelineConfig, FlowPipeline, FlowStream, RollingShutter
    for cfg in (PipelineConfig(), PipelineConfig.node(), PipelineConfig.of_module(), PipelineConfig.evaluate_exp(), PipelineConfig.baseline_1080p()):
        assert cfg.rolling_shutter is None and cfg.rolling_shutter_setting() is None
    rs = RollingShutter(readout=0.9)
    assert values(rs.setting()) == [2, 0, 0.9, 0.5, 1.0]
    assert values(RollingShutter(readout=-0.4, mode="flow", anchor=0.0, rows=960, omega_gain=0.5).setting()) == [1, 960, -0.4, 0.0, 0.5]
    on = PipelineConfig(rolling_shutter=rs)
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params())          # to_params() does not know the setting
    assert PipelineConfig(rolling_shutter=RollingShutter(readout=0.9, mode="off")).rolling_shutter_setting() is None
    with pytest.raises(ValueError):
        PipelineConfig(rolling_shutter=RollingShutter(readout=1.5)).rolling_shutter_setting()
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    Recorder.calls = []
    s = FlowStream(64, 48, batch=1, cfg=PipelineConfig())
    p = FlowPipeline(64, 48, batch=1, cfg=PipelineConfig())
    assert not [c for c in Recorder.calls if c[0] == "set_rolling_shutter"] and callable(s.ideal_points) and callable(p.ideal_points)
    FlowStream(64, 48, batch=1, cfg=on)
    FlowPipeline(64, 48, batch=1, cfg=on)
    sets = [c for c in Recorder.calls if c[0] == "set_rolling_shutter"]
    assert len(sets) == 2 and all(values(c[1][0]) == values(rs.setting()) for c in sets)


def test_optical_fusion_hands_the_setting_to_its_pipeline_config(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig, RollingShutter
    from of_amd.velocity_node import optical_fusion
    assert optical_fusion(spin=False)._rolling_shutter == {}
    node = optical_fusion(spin=False, rolling_shutter=dict(readout=0.9, mode="flow", anchor=0.0))
    rs = node._rolling_shutter["rolling_shutter"]
    assert isinstance(rs, RollingShutter) and values(PipelineConfig(**node._rolling_shutter).rolling_shutter_setting()) == [1, 0, 0.9, 0.0, 1.0]
    given = RollingShutter(readout=-0.3)
    assert optical_fusion(spin=False, rolling_shutter=given)._rolling_shutter["rolling_shutter"] is given
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, rolling_shutter=dict(readout=2.0))
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, rolling_shutter=dict(readout=0.5, exposure=3))


@pytest.mark.gpu
def test_setting_round_trip_every_refusal_and_off_after_null(pkg, ofk):
    ctx = ofk.Context(0, 64, 48, 2, 100, 2)
    try:
        assert values(ctx.get_rolling_shutter()) == [0, 0, 0.0, 0.5, 1.0]          # off
        with pytest.raises(ofk.OfkError) as e:                     # no run with the setting on yet
            ctx.rs_download(1)
        assert e.value.code == ofk.E_INVALID
        good = dict(mode=2, rows=960, readout=-0.7, anchor=0.25, omega_gain=0.5)

        def make(**over):
            d = dict(good, **over)
            return ofk.RShutter(d["mode"], d["rows"], d["readout"], d["anchor"], d["omega_gain"])
        ctx.set_rolling_shutter(make())
        assert values(ctx.get_rolling_shutter()) == values(make())
        nan, inf = float("nan"), float("inf")
        pts = np.zeros((1, 4, 2), np.float32)
        sn = ofk.make_sensors(1)
        for bad in (dict(mode=3), dict(mode=-1), dict(readout=nan), dict(readout=inf), dict(readout=1.0000001), dict(readout=-1.0000001), dict(anchor=nan),
                    dict(anchor=-1e-9), dict(anchor=1.0000001), dict(rows=-1), dict(rows=65537), dict(omega_gain=0.0), dict(omega_gain=nan), dict(omega_gain=inf)):
            for call in (ctx.set_rolling_shutter, lambda m: ctx.rs_correct_points(m, pts, pts, sensors=sn)):
                with pytest.raises(ofk.OfkError) as e:
                    call(make(**bad))
                assert e.value.code == ofk.E_INVALID, bad
            assert values(ctx.get_rolling_shutter()) == values(make()), bad          # the previous setting is in place
        with pytest.raises(ofk.OfkError) as e:                     # gyro mode in the stage entry needs the sensors
            ctx.rs_correct_points(make(), pts, pts)
        assert e.value.code == ofk.E_INVALID
        with pytest.raises(ofk.OfkError):                          # rows 0 = "the run's frame height": there is no run behind a stage entry
            ctx.rs_correct_points(make(rows=0), pts, pts, sensors=sn)
        with pytest.raises(ofk.OfkError):                          # off is no mode for a stage entry
            ctx.rs_correct_points(make(mode=0), pts, pts, sensors=sn)
        assert ctx.rs_correct_points(make(mode=1), pts, pts)[0].shape == (1, 4, 2)      # flow mode needs no sensors
        assert values(ctx.get_rolling_shutter()) == values(make())                        # the stage entry touches no setting
        ctx.set_rolling_shutter(make(rows=0, readout=1.0, anchor=1.0))                    # the ends of every range are inside
        ctx.set_rolling_shutter(make(rows=65536, readout=-1.0, anchor=0.0))
        ctx.set_rolling_shutter(None)
        assert ctx.get_rolling_shutter().mode == 0 and ctx.get_rolling_shutter().rows == 65536
        ctx.set_rolling_shutter(readout=0.25)
        ctx.set_rolling_shutter(ofk.RShutter(0, -9, nan, 7.0, 0.0))                       # mode off: off, whatever else it holds
        assert ctx.get_rolling_shutter().mode == 0 and ctx.get_rolling_shutter().readout == 0.25
        with pytest.raises(ofk.OfkError):
            ctx.rs_download(1)
    finally:
        ctx.close()
