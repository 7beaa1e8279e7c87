"""The depth-per-track entry points exist in the header, the binding and the library; the setting's structure agrees on both sides; the
kernels are in the code object; the pipeline configuration carries the setting with a default that means "off"; optical_fusion hands
it down (CPU-only).  On a device: the setting's defaults, its round trip, every invalid field, and "off" after NULL."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_track_depth", "ofk_get_track_depth", "ofk_track_depth_download", "ofk_track_depth_reset", "ofk_track_depth_step")
FIELDS = [("mode", "int"), ("sigma_flow", "double"), ("b_min", "double"), ("gate", "double"), ("q", "double"), ("min_obs", "int"),
          ("rel_max", "double"), ("min_rows", "int"), ("update", "int")]
NAMES = [n for n, _ in FIELDS]
DEFAULTS = [0.2, 0.5, 3.0, 0.0, 3, 0.25, 8, 1]                   # behind the mode


def values(s):
    return [getattr(s, n) for n in NAMES]


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
        assert s in ofk.SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
    for name, val in (("OFK_TD_OFF", 0), ("OFK_TD_ON", 1), ("OFK_TD_DOUBLES", 32)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
    assert (ofk.TD_OFF, ofk.TD_ON, ofk.TD_DOUBLES) == (0, 1, 32)
    m = re.search(r"typedef struct ofk_track_depth \{(.*?)\} ofk_track_depth;", txt, flags=re.S)
    assert m and re.findall(r"\b(int|double)\s+(\w+);", m.group(1)) == [(t, n) for n, t in FIELDS]
    ctype = {"int": C.c_int, "double": C.c_double}
    assert [(n, t) for n, t in ofk.TrackDepth._fields_] == [(n, ctype[t]) for n, t in FIELDS] and C.sizeof(ofk.TrackDepth) == 64
    assert [getattr(ofk.TrackDepth, n).offset for n in NAMES] == [0, 8, 16, 24, 32, 40, 48, 56, 60]
    assert ("track_depth", ofk.TrackDepth) in ofk.SETTINGS
    assert len(lib.ofk_track_depth_download.argtypes) == 6 and len(lib.ofk_track_depth_reset.argtypes) == 6
    assert len(lib.ofk_track_depth_step.argtypes) == 17
    assert lib.ofk_set_track_depth(None, None) == ofk.E_INVALID and lib.ofk_get_track_depth(None, None) == ofk.E_INVALID
    assert lib.ofk_track_depth_download(None, None, None, None, 1, None) == ofk.E_INVALID
    assert lib.ofk_track_depth_reset(None, 0, None, None, None, 0) == ofk.E_INVALID


def test_depth_kernels_are_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for k in (b"k_track_depth_step", b"k_track_depth_begin", b"k_track_depth_replace", b"k_track_table_update"):
        assert k in blob, k


def test_settings_from_names(built, ofk):
    assert values(ofk.track_depth_setting()) == [1] + DEFAULTS
    t = ofk.track_depth_setting(sigma_flow=0.1, b_min=0.0, gate=0.0, q=1e-6, min_obs=1, rel_max=1.0, min_rows=3, update=False)
    assert values(t) == [1, 0.1, 0.0, 0.0, 1e-6, 1, 1.0, 3, 0]
    assert ofk.track_depth_setting(False, sigma_flow=-1.0).mode == 0          # off: the other fields are not looked at
    for bad in (dict(mode=2), dict(sigma_flow=0.0), dict(sigma_flow=-0.2), dict(b_min=-0.1), dict(gate=-1.0), dict(q=-1e-9), dict(min_obs=0),
                dict(rel_max=0.0), dict(rel_max=-1.0), dict(min_rows=2), dict(sigma_flow=float("nan")), dict(b_min=float("inf")),
                dict(gate=float("nan")), dict(q=float("inf")), dict(rel_max=float("nan"))):
        with pytest.raises(ValueError):
            ofk.track_depth_setting(**bad)
    with pytest.raises(TypeError):
        ofk.track_depth_setting(sigma=3)


class Recorder:
    """Stands in for ofk.Context: records what a pipeline applies to it."""
    calls = []

    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        def f(*a, **k):
            Recorder.calls.append((name, a, k))
        return f


def test_pipeline_config_default_means_off(built, pkg, ofk, monkeypatch):
    from of_amd import pipeline
    from of_amd.pipeline import PipelineConfig, FlowPipeline, FlowStream
    for cfg in (PipelineConfig(), PipelineConfig.node(), PipelineConfig.of_module(), PipelineConfig.evaluate_exp(), PipelineConfig.baseline_1080p()):
        assert cfg.track_depth is None and cfg.track_depth_setting() is None
    assert PipelineConfig(track_depth=False).track_depth_setting() is None
    assert PipelineConfig(track_depth=ofk.track_depth_setting(False)).track_depth_setting() is None
    on = PipelineConfig(track_table=True, track_depth=ofk.track_depth_setting(q=1e-6, min_rows=5))
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params())          # to_params() does not know the setting
    assert values(on.track_depth_setting()) == [1, 0.2, 0.5, 3.0, 1e-6, 3, 0.25, 5, 1]
    assert values(PipelineConfig(track_depth=True).track_depth_setting()) == [1] + DEFAULTS
    with pytest.raises(ValueError):
        PipelineConfig(track_depth="on").track_depth_setting()
    with pytest.raises(ValueError):
        PipelineConfig(track_depth=ofk.TrackDepth(1, 0.2, 0.5, 3.0, 0.0, 3, 0.25, 2, 1)).track_depth_setting()
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    Recorder.calls = []
    s = FlowStream(64, 48, batch=1, cfg=PipelineConfig())
    FlowPipeline(64, 48, batch=1, cfg=on)                        # frame pairs ignore the setting
    assert not [c for c in Recorder.calls if c[0] == "set_track_depth"] and callable(s.depths)
    FlowStream(64, 48, batch=1, cfg=on)
    names = [c[0] for c in Recorder.calls]
    sets = [c for c in Recorder.calls if c[0] == "set_track_depth"]
    assert len(sets) == 1 and values(sets[0][1][0]) == [1, 0.2, 0.5, 3.0, 1e-6, 3, 0.25, 5, 1]
    assert names.index("set_track_table") < names.index("set_track_depth")        # one settings path, the table first


def test_optical_fusion_hands_the_depth_setting_to_its_pipeline_config(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    from of_amd.velocity_node import optical_fusion
    plain = optical_fusion(spin=False)
    assert plain._track_depth == {} and plain._track_table == {} and plain.last_track_depth is None
    node = optical_fusion(spin=False, track_depth=dict(q=1e-6, gate=2.5))
    assert values(PipelineConfig(**node._track_depth).track_depth_setting()) == [1, 0.2, 0.5, 2.5, 1e-6, 3, 0.25, 8, 1]
    assert node._track_table == dict(track_table=True)           # the depths need the table
    both = optical_fusion(spin=False, track_depth=True, track_table=dict(seed="flow"))
    assert both._track_depth == dict(track_depth=True) and both._track_table["track_table"].seed == ofk.TT_SEED_FLOW
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, track_depth=dict(min_rows=1))
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, track_depth=dict(sigma=3))
    from of_amd import simulation, velocity_node
    assert callable(simulation.track_depth_step) and callable(velocity_node.track_depth_step)


@pytest.mark.gpu
def test_setting_round_trip_invalid_fields_and_off_after_null(pkg, ofk):
    ctx = ofk.Context(0, 64, 48, 2, 100, 2)
    try:
        assert values(ctx.get_track_depth()) == [0] + DEFAULTS   # off, the defaults behind it
        ctx.set_track_depth(sigma_flow=0.3, b_min=0.0, gate=0.0, q=1e-7, min_obs=1, rel_max=0.5, min_rows=3, update=False)
        good = [1, 0.3, 0.0, 0.0, 1e-7, 1, 0.5, 3, 0]
        assert values(ctx.get_track_depth()) == good
        nan, inf = float("nan"), float("inf")
        for bad in (dict(mode=2), dict(mode=-1), dict(sigma_flow=0.0), dict(sigma_flow=-0.3), dict(sigma_flow=nan), dict(sigma_flow=inf),
                    dict(b_min=-1e-9), dict(b_min=nan), dict(b_min=inf), dict(gate=-1.0), dict(gate=nan), dict(gate=inf), dict(q=-1e-12), dict(q=nan),
                    dict(q=inf), dict(min_obs=0), dict(min_obs=-3), dict(rel_max=0.0), dict(rel_max=-0.25), dict(rel_max=nan), dict(rel_max=inf),
                    dict(min_rows=2), dict(min_rows=0)):
            with pytest.raises(ofk.OfkError) as e:
                ctx.set_track_depth(ofk.TrackDepth(*[dict(zip(NAMES, good), **bad)[n] for n in NAMES]))
            assert e.value.code == ofk.E_INVALID, bad
            assert values(ctx.get_track_depth()) == good, bad    # the previous setting is in place
        ctx.set_track_depth(None)
        assert ctx.get_track_depth().mode == 0 and values(ctx.get_track_depth())[1:] == good[1:]
        ctx.set_track_depth(q=1e-5)
        ctx.set_track_depth(ofk.TrackDepth(0, -9.0, -9.0, -9.0, -9.0, -9, -9.0, -9, -9))        # mode off: off, whatever else the structure holds
        assert ctx.get_track_depth().mode == 0 and ctx.get_track_depth().q == 1e-5
        with pytest.raises(ofk.OfkError):                          # nothing has stepped with the setting on
            ctx.track_depth_download(2)
        with pytest.raises(ofk.OfkError):                          # no active stream
            ctx.track_depth_reset(0, [0.5], [0.01], [1])
    finally:
        ctx.close()
