"""The keyframe's entry points exist in the header, the binding and the library; the setting's structure agrees on both sides; the
kernels are in the code object; the pipeline configuration carries the setting with a default that means "off"; optical_fusion hands
it down (CPU-only).  On a device: the setting's defaults, its round trip, every invalid field, "off" after NULL, download and reset
before any step."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_keyframe", "ofk_get_keyframe", "ofk_keyframe_download", "ofk_keyframe_reset", "ofk_keyframe_step")
FIELDS = [("mode", "int"), ("sigma_flow", "double"), ("gate", "double"), ("min_rows", "int"), ("min_share", "double"), ("rot_max", "double"),
          ("max_age", "int")]
NAMES = [n for n, _ in FIELDS]
DEFAULTS = [0.2, 2.0, 8, 0.5, 0.5, 0]                             # behind the mode
CONSTANTS = (("OFK_KEY_OFF", 0), ("OFK_KEY_ON", 1), ("OFK_KEY_DOUBLES", 32), ("OFK_KEY_STATE", 16), ("OFK_KEY_INTS", 4), ("OFK_KEY_SOLVED", 0),
             ("OFK_KEY_UNSOLVED", 1), ("OFK_KEY_NONE", 2), ("OFK_KEY_RE_FLAG", 1), ("OFK_KEY_RE_ROWS", 2), ("OFK_KEY_RE_SHARE", 3),
             ("OFK_KEY_RE_ANGLE", 4), ("OFK_KEY_RE_AGE", 5))


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
    for name, val in CONSTANTS:
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
        assert getattr(ofk, name[4:]) == val, name
    assert re.search(r"#define\s+OFK_KEY_MIN_DEPTH\s+0\.1\b", txt) and ofk.KEY_MIN_DEPTH == 0.1
    m = re.search(r"typedef struct ofk_keyframe \{(.*?)\} ofk_keyframe;", txt, flags=re.S)
    assert m and re.findall(r"\b(int|double)\s+(\w+);", m.group(1)) == [(t, n) for n, t in FIELDS]
    ctype = {"int": C.c_int, "double": C.c_double}
    assert [(n, t) for n, t in ofk.Keyframe._fields_] == [(n, ctype[t]) for n, t in FIELDS] and C.sizeof(ofk.Keyframe) == 56
    assert [getattr(ofk.Keyframe, n).offset for n in NAMES] == [0, 8, 16, 24, 32, 40, 48]
    assert ("keyframe", ofk.Keyframe) in ofk.SETTINGS
    assert len(lib.ofk_keyframe_download.argtypes) == 6 and len(lib.ofk_keyframe_reset.argtypes) == 3
    assert len(lib.ofk_keyframe_step.argtypes) == 18
    assert lib.ofk_set_keyframe(None, None) == ofk.E_INVALID and lib.ofk_get_keyframe(None, None) == ofk.E_INVALID
    assert lib.ofk_keyframe_download(None, None, None, 1, None, None) == ofk.E_INVALID
    assert lib.ofk_keyframe_reset(None, 0, None) == ofk.E_INVALID


def test_keyframe_kernels_are_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for k in (b"k_keyframe_step", b"k_keyframe_begin", b"k_keyframe_replace", b"k_keyframe_reset", b"k_track_table_update"):
        assert k in blob, k


def test_settings_from_names(built, ofk):
    assert values(ofk.keyframe_setting()) == [1] + DEFAULTS
    k = ofk.keyframe_setting(sigma_flow=0.1, gate=0.0, min_rows=3, min_share=1.0, rot_max=0.1, max_age=50)
    assert values(k) == [1, 0.1, 0.0, 3, 1.0, 0.1, 50]
    assert ofk.keyframe_setting(False, sigma_flow=-1.0).mode == 0             # off: the other fields are not looked at
    nan, inf = float("nan"), float("inf")
    for bad in (dict(mode=2), dict(sigma_flow=0.0), dict(sigma_flow=-0.2), dict(gate=-1.0), dict(min_rows=2), dict(min_share=-0.1),
                dict(min_share=1.1), dict(rot_max=0.0), dict(rot_max=-1.0), dict(max_age=-1), dict(sigma_flow=nan), dict(gate=inf),
                dict(min_share=nan), dict(rot_max=inf)):
        with pytest.raises(ValueError):
            ofk.keyframe_setting(**bad)
    with pytest.raises(TypeError):
        ofk.keyframe_setting(sigma=3)


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
        assert cfg.keyframe is None and cfg.keyframe_setting() is None
    assert PipelineConfig(keyframe=False).keyframe_setting() is None
    assert PipelineConfig(keyframe=ofk.keyframe_setting(False)).keyframe_setting() is None
    on = PipelineConfig(track_table=True, keyframe=ofk.keyframe_setting(min_share=0.7, max_age=100))
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params())          # to_params() does not know the setting
    assert values(on.keyframe_setting()) == [1, 0.2, 2.0, 8, 0.7, 0.5, 100]
    assert values(PipelineConfig(keyframe=True).keyframe_setting()) == [1] + DEFAULTS
    with pytest.raises(ValueError):
        PipelineConfig(keyframe="on").keyframe_setting()
    with pytest.raises(ValueError):
        PipelineConfig(keyframe=ofk.Keyframe(1, 0.2, 2.0, 2, 0.5, 0.5, 0)).keyframe_setting()
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    Recorder.calls = []
    s = FlowStream(64, 48, batch=1, cfg=PipelineConfig())
    FlowPipeline(64, 48, batch=1, cfg=on)                        # frame pairs ignore the setting
    assert not [c for c in Recorder.calls if c[0] == "set_keyframe"] and callable(s.position)
    FlowStream(64, 48, batch=1, cfg=on)
    names = [c[0] for c in Recorder.calls]
    sets = [c for c in Recorder.calls if c[0] == "set_keyframe"]
    assert len(sets) == 1 and values(sets[0][1][0]) == [1, 0.2, 2.0, 8, 0.7, 0.5, 100]
    assert names.index("set_track_table") < names.index("set_keyframe")           # one settings path, the table first


def test_optical_fusion_hands_the_keyframe_setting_to_its_pipeline_config(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    from of_amd.velocity_node import optical_fusion
    plain = optical_fusion(spin=False)
    assert plain._keyframe == {} and plain._track_table == {} and plain.last_keyframe is None
    node = optical_fusion(spin=False, keyframe=dict(min_share=0.7, gate=1.5))
    assert values(PipelineConfig(**node._keyframe).keyframe_setting()) == [1, 0.2, 1.5, 8, 0.7, 0.5, 0]
    assert node._track_table == dict(track_table=True)           # the keyframe needs the table
    both = optical_fusion(spin=False, keyframe=True, track_table=dict(seed="flow"))
    assert both._keyframe == dict(keyframe=True) and both._track_table["track_table"].seed == ofk.TT_SEED_FLOW
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, keyframe=dict(min_rows=1))
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, keyframe=dict(sigma=3))
    from of_amd import simulation, velocity_node
    assert callable(simulation.keyframe_step) and callable(velocity_node.keyframe_step)


@pytest.mark.gpu
def test_setting_round_trip_invalid_fields_off_after_null_download_and_reset_before_a_step(pkg, ofk):
    ctx = ofk.Context(0, 64, 48, 2, 100, 2)
    try:
        assert values(ctx.get_keyframe()) == [0] + DEFAULTS      # off, the defaults behind it
        ctx.set_keyframe(sigma_flow=0.3, gate=0.0, min_rows=3, min_share=1.0, rot_max=0.25, max_age=7)
        good = [1, 0.3, 0.0, 3, 1.0, 0.25, 7]
        assert values(ctx.get_keyframe()) == good
        nan, inf = float("nan"), float("inf")
        for bad in (dict(mode=2), dict(mode=-1), dict(sigma_flow=0.0), dict(sigma_flow=-0.3), dict(sigma_flow=nan), dict(sigma_flow=inf),
                    dict(gate=-1.0), dict(gate=nan), dict(gate=inf), dict(min_rows=2), dict(min_rows=0), dict(min_share=-1e-9),
                    dict(min_share=1.0 + 1e-9), dict(min_share=nan), dict(min_share=inf), dict(rot_max=0.0), dict(rot_max=-0.5), dict(rot_max=nan),
                    dict(rot_max=inf), dict(max_age=-1)):
            with pytest.raises(ofk.OfkError) as e:
                ctx.set_keyframe(ofk.Keyframe(*[dict(zip(NAMES, good), **bad)[n] for n in NAMES]))
            assert e.value.code == ofk.E_INVALID, bad
            assert values(ctx.get_keyframe()) == good, bad       # the previous setting is in place
        ctx.set_keyframe(None)
        assert ctx.get_keyframe().mode == 0 and values(ctx.get_keyframe())[1:] == good[1:]
        ctx.set_keyframe(max_age=9)
        ctx.set_keyframe(ofk.Keyframe(0, -9.0, -9.0, -9, -9.0, -9.0, -9))     # mode off: off, whatever else the structure holds
        assert ctx.get_keyframe().mode == 0 and ctx.get_keyframe().max_age == 9
        with pytest.raises(ofk.OfkError):                          # nothing has stepped with the setting on
            ctx.keyframe_download(2)
        with pytest.raises(ofk.OfkError):                          # no active stream
            ctx.keyframe_reset(0, [1.0, 2.0, 3.0])
    finally:
        ctx.close()
