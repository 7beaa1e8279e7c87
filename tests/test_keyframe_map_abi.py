"""The keyframe map's entry points exist in the header, the binding and the library; the setting's structure agrees on both sides; the
kernels are in the code object; the pipeline configuration carries the setting with a default that means "off"; optical_fusion hands
it down (CPU-only).  On a device: the setting's defaults, its round trip, every invalid field leaving the setting as it was, "off"
after NULL."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_keyframe_map", "ofk_get_keyframe_map", "ofk_keyframe_map_download", "ofk_keyframe_map_step")
NAMES = ["mode", "min_obs", "rel_max", "min_rows", "ready_share", "weights"]
DEFAULTS = [3, 0.02, 8, 0.5, 1]                                  # behind the mode
CONSTANTS = (("OFK_KEYMAP_OFF", 0), ("OFK_KEYMAP_ON", 1), ("OFK_KEYMAP_DOUBLES", 32), ("OFK_KEYMAP_USED", 0), ("OFK_KEYMAP_NONE", 1),
             ("OFK_KEYMAP_FEW", 2), ("OFK_KEYMAP_FELL_BACK", 3), ("OFK_KEY_RE_MAP", 6))


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
    m = re.search(r"typedef struct ofk_keyframe_map \{(.*?)\} ofk_keyframe_map;", txt, flags=re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == \
        "int mode; int min_obs; double rel_max; int min_rows; double ready_share; int weights;"
    want = [("mode", C.c_int), ("min_obs", C.c_int), ("rel_max", C.c_double), ("min_rows", C.c_int), ("ready_share", C.c_double),
            ("weights", C.c_int)]
    assert list(ofk.KeyframeMap._fields_) == want and C.sizeof(ofk.KeyframeMap) == 40
    assert [getattr(ofk.KeyframeMap, n).offset for n in NAMES] == [0, 4, 8, 16, 24, 32]
    assert ("keyframe_map", ofk.KeyframeMap) in ofk.SETTINGS
    assert len(lib.ofk_keyframe_map_download.argtypes) == 5
    assert len(lib.ofk_keyframe_map_step.argtypes) == len(lib.ofk_keyframe_step.argtypes) + 8   # the setting, three depth arrays, four of the map
    assert lib.ofk_set_keyframe_map(None, None) == ofk.E_INVALID and lib.ofk_get_keyframe_map(None, None) == ofk.E_INVALID
    assert lib.ofk_keyframe_map_download(None, None, None, 1, None) == ofk.E_INVALID


def test_map_kernels_are_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for k in (b"k_keyframe_step_map", b"k_keymap_clear", b"k_keyframe_step_rot", b"k_keyframe_step"):
        assert k in blob, k


def test_settings_from_names(built, ofk):
    assert values(ofk.keyframe_map_setting()) == [1] + DEFAULTS
    m = ofk.keyframe_map_setting(min_obs=5, rel_max=0.05, min_rows=12, ready_share=0.0, weights=0)
    assert values(m) == [1, 5, 0.05, 12, 0.0, 0]
    assert ofk.keyframe_map_setting(False, rel_max=-1.0).mode == 0      # off: the other fields are not looked at
    nan, inf = float("nan"), float("inf")
    for bad in (dict(mode=2), dict(min_obs=0), dict(rel_max=0.0), dict(rel_max=-0.1), dict(rel_max=nan), dict(rel_max=inf), dict(min_rows=2),
                dict(ready_share=-0.1), dict(ready_share=1.1), dict(ready_share=nan), dict(weights=2), dict(weights=-1)):
        with pytest.raises(ValueError):
            ofk.keyframe_map_setting(**bad)
    with pytest.raises(TypeError):
        ofk.keyframe_map_setting(sigma=3)


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
    from of_amd.pipeline import PipelineConfig, FlowStream
    for cfg in (PipelineConfig(), PipelineConfig.node(), PipelineConfig.baseline_1080p(), PipelineConfig(keyframe=True, track_depth=True)):
        assert cfg.keyframe_map is None and cfg.keyframe_map_setting() is None
    assert PipelineConfig(keyframe=True, track_depth=True, keyframe_map=False).keyframe_map_setting() is None
    assert PipelineConfig(keyframe_map=ofk.keyframe_map_setting(False)).keyframe_map_setting() is None
    on = PipelineConfig(track_table=True, track_depth=True, keyframe=True, keyframe_map=ofk.keyframe_map_setting(rel_max=0.05, min_rows=10))
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params())
    assert values(on.keyframe_map_setting()) == [1, 3, 0.05, 10, 0.5, 1]
    assert values(PipelineConfig(keyframe=True, track_depth=True, keyframe_map=True).keyframe_map_setting()) == [1] + DEFAULTS
    with pytest.raises(ValueError):
        PipelineConfig(keyframe=True, track_depth=True, keyframe_map="on").keyframe_map_setting()
    with pytest.raises(ValueError):                                # the map is the depths', frozen at the keyframe: it needs both
        PipelineConfig(keyframe=True, keyframe_map=True).keyframe_map_setting()
    with pytest.raises(ValueError):
        PipelineConfig(track_depth=True, keyframe_map=True).keyframe_map_setting()
    with pytest.raises(ValueError):                                # the joint solve over map rows is not built
        PipelineConfig(keyframe=True, track_depth=True, keyframe_rotation=True, keyframe_map=True).keyframe_map_setting()
    with pytest.raises(ValueError):
        PipelineConfig(keyframe=True, track_depth=True, keyframe_map=ofk.KeyframeMap(1, 0, 0.02, 8, 0.5, 1)).keyframe_map_setting()
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    Recorder.calls = []
    s = FlowStream(64, 48, batch=1, cfg=PipelineConfig(track_table=True, track_depth=True, keyframe=True))
    assert not [c for c in Recorder.calls if c[0] == "set_keyframe_map"] and callable(s.key_map)
    FlowStream(64, 48, batch=1, cfg=on)
    names = [c[0] for c in Recorder.calls]
    sets = [c for c in Recorder.calls if c[0] == "set_keyframe_map"]
    assert len(sets) == 1 and values(sets[0][1][0]) == [1, 3, 0.05, 10, 0.5, 1]
    assert names.index("set_keyframe") < names.index("set_keyframe_map") and names.index("set_track_depth") < names.index("set_keyframe_map")
    Recorder.calls = []                                            # independent pairs have no keyframe: FlowPipeline ignores the setting
    pipeline.FlowPipeline(64, 48, batch=1, cfg=on)
    assert not [c for c in Recorder.calls if c[0] == "set_keyframe_map"]


def test_optical_fusion_hands_the_setting_to_its_pipeline_config(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    from of_amd.velocity_node import optical_fusion
    plain = optical_fusion(spin=False, keyframe=True)
    assert plain._keyframe_map == {} and plain.last_key_map is None
    node = optical_fusion(spin=False, keyframe_map=dict(rel_max=0.05, weights=0))      # it switches the keyframe, the depths and the table on
    assert node._keyframe and node._track_depth and node._track_table
    cfg = PipelineConfig(**node._track_table, **node._track_depth, **node._keyframe, **node._keyframe_map)
    assert values(cfg.keyframe_map_setting()) == [1, 3, 0.05, 8, 0.5, 0]
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, keyframe_map=dict(min_rows=2))
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, keyframe_rotation=True, keyframe_map=True)
    from of_amd import simulation, velocity_node
    assert callable(simulation.keyframe_map_step) and callable(velocity_node.keyframe_map_step)


@pytest.mark.gpu
def test_setting_round_trip_and_every_refusal_leaves_it_as_it_was(pkg, ofk):
    ctx = ofk.Context(0, 64, 48, 2, 100, 2)
    try:
        assert values(ctx.get_keyframe_map()) == [0] + DEFAULTS     # off, the defaults behind it
        good = [1, 5, 0.05, 12, 0.25, 0]
        ctx.set_keyframe_map(ofk.KeyframeMap(*good))
        assert values(ctx.get_keyframe_map()) == good
        nan, inf = float("nan"), float("inf")
        for bad in (dict(mode=2), dict(mode=-1), dict(min_obs=0), dict(min_obs=-3), dict(rel_max=0.0), dict(rel_max=-0.1), dict(rel_max=nan),
                    dict(rel_max=inf), dict(min_rows=2), dict(ready_share=-0.1), dict(ready_share=1.5), dict(ready_share=nan), dict(ready_share=inf),
                    dict(weights=2), dict(weights=-1)):
            with pytest.raises(ofk.OfkError) as e:
                ctx.set_keyframe_map(ofk.KeyframeMap(*[dict(zip(NAMES, good), **bad)[n] for n in NAMES]))
            assert e.value.code == ofk.E_INVALID, bad
            assert values(ctx.get_keyframe_map()) == good, bad     # the previous setting is in place
        ctx.set_keyframe_map(None)
        assert ctx.get_keyframe_map().mode == 0 and values(ctx.get_keyframe_map())[1:] == good[1:]
        ctx.set_keyframe_map(min_rows=9)
        ctx.set_keyframe_map(ofk.KeyframeMap(0, -9, -9.0, -9, -9.0, -9))       # mode off: off, whatever else it holds
        assert ctx.get_keyframe_map().mode == 0 and ctx.get_keyframe_map().min_rows == 9
        with pytest.raises(ofk.OfkError):                          # nothing has stepped with the setting on
            ctx.keyframe_map_download(2)
    finally:
        ctx.close()
