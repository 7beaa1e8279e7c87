"""The position filter's entry points exist in the header, the binding and the library; the setting's structure agrees on both sides;
the kernels are in the code object; the pipeline configuration carries the setting with a default that means "off"; optical_fusion
hands it down (CPU-only).  On a device: the setting's defaults, its round trip, every invalid field, "off" after NULL, download, reset
and input before any step."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_pos_filter", "ofk_get_pos_filter", "ofk_pos_filter_input", "ofk_pos_filter_reset", "ofk_pos_filter_download", "ofk_pos_filter_step")
NAMES = ["mode", "dt", "sigma_v", "floor", "infl", "share", "q_p", "q_v", "q_b", "p0_p", "p0_v", "p0_b", "nis_max"]
DEFAULTS = [1.0, 1e-3, 0.0, 1.0, 0.5, 0.0, 1e-3, 0.0, 0.0, 1.0, 0.0, 0.0]       # behind the mode
CONSTANTS = (("OFK_POSF_OFF", 0), ("OFK_POSF_ON", 1), ("OFK_POSF_STATES", 12), ("OFK_POSF_INPUT", 12), ("OFK_POSF_INTS", 16), ("OFK_POSF_DOUBLES", 48),
             ("OFK_POSF_NOT", 0), ("OFK_POSF_APPLIED", 1), ("OFK_POSF_GATED", 2), ("OFK_POSF_REFUSED", 3))


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
    m = re.search(r"typedef struct ofk_pos_filter \{(.*?)\} ofk_pos_filter;", txt, flags=re.S)
    assert m and re.fullmatch(r"\s*int mode;\s*double ([\w, ]+);\s*", m.group(1))
    assert ["mode"] + [n.strip() for n in re.search(r"double ([\w, ]+);", m.group(1)).group(1).split(",")] == NAMES
    assert [(n, t) for n, t in ofk.PosFilter._fields_] == [("mode", C.c_int)] + [(n, C.c_double) for n in NAMES[1:]]
    assert C.sizeof(ofk.PosFilter) == 104 and [getattr(ofk.PosFilter, n).offset for n in NAMES] == [0] + list(range(8, 104, 8))
    assert ("pos_filter", ofk.PosFilter) in ofk.SETTINGS
    assert [len(getattr(lib, s).argtypes) for s in NEW] == [2, 2, 2, 3, 5, 12]
    assert lib.ofk_set_pos_filter(None, None) == ofk.E_INVALID and lib.ofk_get_pos_filter(None, None) == ofk.E_INVALID
    assert lib.ofk_pos_filter_input(None, None) == ofk.E_INVALID and lib.ofk_pos_filter_reset(None, 0, None) == ofk.E_INVALID
    assert lib.ofk_pos_filter_download(None, None, None, None, None) == ofk.E_INVALID
    assert lib.ofk_pos_filter_step(None, None, None, None, None, None, None, None, None, None, 1, None) == ofk.E_INVALID


def test_pos_filter_kernels_are_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for k in (b"k_pos_filter_step", b"k_pos_filter_clear", b"k_keyframe_step"):
        assert k in blob, k


def test_settings_from_names(built, ofk):
    assert values(ofk.pos_filter_setting()) == [1] + DEFAULTS
    f = ofk.pos_filter_setting(dt=0.02, sigma_v=0.0, floor=1e-4, infl=2.0, share=1.0, q_p=1e-5, q_v=0.0, q_b=1e-6, p0_p=3.0, p0_v=0.0, p0_b=0.1, nis_max=16)
    assert values(f) == [1, 0.02, 0.0, 1e-4, 2.0, 1.0, 1e-5, 0.0, 1e-6, 3.0, 0.0, 0.1, 16.0]
    assert ofk.pos_filter_setting(False, dt=-1.0).mode == 0                  # off: the other fields are not looked at
    nan, inf = float("nan"), float("inf")
    for bad in [dict(mode=2), dict(dt=0.0), dict(dt=-1.0), dict(infl=0.0), dict(infl=-1.0), dict(share=-0.1), dict(share=1.1), dict(nis_max=-1.0)] + \
               [{n: -1e-9} for n in ("sigma_v", "floor", "q_p", "q_v", "q_b", "p0_p", "p0_v", "p0_b")] + [{n: v} for n in NAMES[1:] for v in (nan, inf)]:
        with pytest.raises(ValueError):
            ofk.pos_filter_setting(**bad)
    with pytest.raises(TypeError):
        ofk.pos_filter_setting(sigma=3)


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
        assert cfg.pos_filter is None and cfg.pos_filter_setting() is None
    assert PipelineConfig(pos_filter=False).pos_filter_setting() is None
    assert PipelineConfig(pos_filter=ofk.pos_filter_setting(False)).pos_filter_setting() is None
    on = PipelineConfig(track_table=True, keyframe=True, pos_filter=ofk.pos_filter_setting(share=0.25, nis_max=9))
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params())          # to_params() does not know the setting
    assert values(on.pos_filter_setting()) == [1, 1.0, 1e-3, 0.0, 1.0, 0.25, 0.0, 1e-3, 0.0, 0.0, 1.0, 0.0, 9.0]
    assert values(PipelineConfig(keyframe=True, pos_filter=True).pos_filter_setting()) == [1] + DEFAULTS
    with pytest.raises(ValueError):                              # it fuses the keyframe's displacement
        PipelineConfig(pos_filter=True).pos_filter_setting()
    with pytest.raises(ValueError):
        PipelineConfig(keyframe=True, pos_filter="on").pos_filter_setting()
    with pytest.raises(ValueError):
        PipelineConfig(keyframe=True, pos_filter=ofk.PosFilter(1, 0.0, *DEFAULTS[1:])).pos_filter_setting()
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    Recorder.calls = []
    s = FlowStream(64, 48, batch=1, cfg=PipelineConfig())
    FlowPipeline(64, 48, batch=1, cfg=on)                        # frame pairs ignore the setting
    assert not [c for c in Recorder.calls if c[0] == "set_pos_filter"] and callable(s.fused_position) and callable(s.position_input)
    fs = FlowStream(64, 48, batch=2, cfg=on)
    names = [c[0] for c in Recorder.calls]
    sets = [c for c in Recorder.calls if c[0] == "set_pos_filter"]
    assert len(sets) == 1 and values(sets[0][1][0])[5] == 0.25
    assert names.index("set_track_table") < names.index("set_keyframe") < names.index("set_pos_filter")      # one settings path
    fs.position_input(du=[1e-3, 0, 0], fix=[[1.0, 2.0, 3.0], [np.nan, 0, 0]], fix_sigma=0.05)
    row = [c for c in Recorder.calls if c[0] == "pos_filter_input"][-1][1][0]
    assert np.array_equal(row[:, 0:3], [[1e-3, 0, 0]] * 2) and np.array_equal(row[:, 3], [1, 0]) and np.array_equal(row[0, 4:10], [1, 2, 3, .05, .05, .05])
    assert not row[1, 4:7].any()
    with pytest.raises(ValueError):
        fs.position_input(fix=[1.0, 2.0, 3.0])


def test_optical_fusion_hands_the_pos_filter_setting_to_its_pipeline_config(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    from of_amd.velocity_node import optical_fusion
    plain = optical_fusion(spin=False)
    assert plain._pos_filter == {} and plain._keyframe == {} and plain._track_table == {} and plain.last_position is None
    node = optical_fusion(spin=False, pos_filter=dict(share=0.25, nis_max=16))
    assert values(PipelineConfig(**node._keyframe, **node._pos_filter).pos_filter_setting())[5] == 0.25
    assert node._keyframe == dict(keyframe=True) and node._track_table == dict(track_table=True)     # it needs both
    both = optical_fusion(spin=False, pos_filter=True, keyframe=dict(min_share=0.7))
    assert both._pos_filter == dict(pos_filter=True) and both._keyframe["keyframe"].min_share == 0.7
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, pos_filter=dict(share=2.0))
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, pos_filter=dict(sigma=3))
    with pytest.raises(ValueError):                              # the keyframe switched off by hand
        optical_fusion(spin=False, pos_filter=True, keyframe=False)
    node.call_fix([1.0, 2.0, 3.0], 0.05)
    assert np.array_equal(node._fix[0], [1, 2, 3]) and np.array_equal(node._fix[1], [0.05] * 3)
    for bad in (([np.nan, 0, 0], 0.05), ([0, 0, 0], 0.0), ([0, 0, 0], [0.1, np.inf, 0.1])):
        with pytest.raises(ValueError):
            node.call_fix(*bad)
    with pytest.raises(ValueError):
        plain.call_fix([0, 0, 0], 0.05)
    from of_amd import simulation, velocity_node
    assert callable(simulation.pos_filter_step) and callable(velocity_node.pos_filter_step)


@pytest.mark.gpu
def test_setting_round_trip_invalid_fields_off_after_null_download_reset_and_input_before_a_step(pkg, ofk):
    ctx = ofk.Context(0, 64, 48, 2, 100, 2)
    try:
        assert values(ctx.get_pos_filter()) == [0] + DEFAULTS    # off, the defaults behind it
        good = [1, 0.02, 2e-3, 1e-4, 2.0, 0.25, 1e-5, 2e-3, 1e-6, 3.0, 0.5, 0.1, 16.0]
        ctx.set_pos_filter(**dict(zip(NAMES[1:], good[1:])))
        assert values(ctx.get_pos_filter()) == good
        nan, inf = float("nan"), float("inf")
        bads = [dict(mode=2), dict(mode=-1), dict(dt=0.0), dict(dt=-0.02), dict(infl=0.0), dict(infl=-2.0), dict(share=-1e-9), dict(share=1.0 + 1e-9),
                dict(nis_max=-1.0)]
        bads += [{n: -1e-9} for n in ("sigma_v", "floor", "q_p", "q_v", "q_b", "p0_p", "p0_v", "p0_b")]
        bads += [{n: v} for n in NAMES[1:] for v in (nan, inf, -inf)]
        for bad in bads:
            with pytest.raises(ofk.OfkError) as e:
                ctx.set_pos_filter(ofk.PosFilter(*[dict(zip(NAMES, good), **bad)[n] for n in NAMES]))
            assert e.value.code == ofk.E_INVALID, bad
            assert values(ctx.get_pos_filter()) == good, bad     # the previous setting is in place
        ctx.set_pos_filter(None)
        assert ctx.get_pos_filter().mode == 0 and values(ctx.get_pos_filter())[1:] == good[1:]
        ctx.set_pos_filter(nis_max=4.0)
        ctx.set_pos_filter(ofk.PosFilter(0, *[-9.0] * 12))       # mode off: off, whatever else the structure holds
        assert ctx.get_pos_filter().mode == 0 and ctx.get_pos_filter().nis_max == 4.0
        with pytest.raises(ofk.OfkError):                          # nothing has stepped with the setting on
            ctx.pos_filter_download(2)
        with pytest.raises(ofk.OfkError):                          # no active stream
            ctx.pos_filter_reset(0, [1.0, 2.0, 3.0])
        with pytest.raises(ofk.OfkError):
            ctx.pos_filter_input(np.zeros((2, 12)))
    finally:
        ctx.close()
