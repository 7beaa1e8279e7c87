"""The keyframe rotation's entry points exist in the header, the binding and the library; the setting's structure agrees on both sides;
the kernels are in the code object; the pipeline configuration carries the setting with a default that means "off"; optical_fusion
hands it down (CPU-only).  On a device: the setting's defaults, its round trip, every invalid field leaving the setting as it was,
"off" after NULL."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_keyframe_rotation", "ofk_get_keyframe_rotation", "ofk_keyframe_rotation_download", "ofk_keyframe_rotation_step")
NAMES = ["mode", "source", "axes", "sigma_gyro", "sigma_bias", "sigma_att", "iters", "delta_max"]
DEFAULTS = [0, [1, 1, 1], 0.0, 1e-4, 1e-3, 2, 0.1]               # behind the mode
CONSTANTS = (("OFK_KEYROT_OFF", 0), ("OFK_KEYROT_ON", 1), ("OFK_KEYROT_GYRO", 0), ("OFK_KEYROT_ATTITUDE", 1), ("OFK_KEYROT_DOUBLES", 40),
             ("OFK_KEYROT_STATE", 12), ("OFK_KEYROT_MAX_ITERS", 8), ("OFK_KEYROT_OK", 0), ("OFK_KEYROT_NONE", 1), ("OFK_KEYROT_SINGULAR", 2),
             ("OFK_KEYROT_LARGE", 3), ("OFK_KEYROT_HELD", 4))


def values(s):
    return [list(getattr(s, n)) if n == "axes" else getattr(s, n) for n in NAMES]


def make(ofk, v):
    return ofk.KeyframeRotation(v[0], v[1], (C.c_int * 3)(*v[2]), *v[3:])


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
    m = re.search(r"typedef struct ofk_keyframe_rotation \{(.*?)\} ofk_keyframe_rotation;", txt, flags=re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == \
        "int mode; int source; int axes[3]; double sigma_gyro, sigma_bias, sigma_att; int iters; double delta_max;"
    want = [("mode", C.c_int), ("source", C.c_int), ("axes", C.c_int * 3), ("sigma_gyro", C.c_double), ("sigma_bias", C.c_double),
            ("sigma_att", C.c_double), ("iters", C.c_int), ("delta_max", C.c_double)]
    assert list(ofk.KeyframeRotation._fields_) == want and C.sizeof(ofk.KeyframeRotation) == 64
    assert [getattr(ofk.KeyframeRotation, n).offset for n in NAMES] == [0, 4, 8, 24, 32, 40, 48, 56]
    assert ("keyframe_rotation", ofk.KeyframeRotation) in ofk.SETTINGS
    assert len(lib.ofk_keyframe_rotation_download.argtypes) == 2 and len(lib.ofk_keyframe_rotation_step.argtypes) == 21
    assert len(lib.ofk_keyframe_step.argtypes) == 18             # ofk_keyframe_step's arguments, then rstate and rrec
    assert lib.ofk_set_keyframe_rotation(None, None) == ofk.E_INVALID and lib.ofk_get_keyframe_rotation(None, None) == ofk.E_INVALID
    assert lib.ofk_keyframe_rotation_download(None, None) == ofk.E_INVALID


def test_rotation_kernels_are_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for k in (b"k_keyframe_step_rot", b"k_keyrot_clear", b"k_keyframe_step"):
        assert k in blob, k


def test_settings_from_names(built, ofk):
    assert values(ofk.keyframe_rotation_setting()) == [1] + DEFAULTS
    r = ofk.keyframe_rotation_setting(source="attitude", axes=(1, 0, 1), sigma_gyro=1e-5, sigma_bias=0.0, sigma_att=2e-3, iters=1, delta_max=0.05)
    assert values(r) == [1, 1, [1, 0, 1], 1e-5, 0.0, 2e-3, 1, 0.05]
    assert values(ofk.keyframe_rotation_setting(sigma_bias=float("inf")))[4] == float("inf")      # free
    assert ofk.keyframe_rotation_setting(False, sigma_att=-1.0).mode == 0      # off: the other fields are not looked at
    nan, inf = float("nan"), float("inf")
    for bad in (dict(mode=2), dict(source="star"), dict(source=2), dict(sigma_gyro=-1e-9), dict(sigma_bias=-1.0), dict(sigma_att=-1.0),
                dict(sigma_gyro=nan), dict(sigma_bias=nan), dict(sigma_att=nan), dict(sigma_att=inf), dict(iters=0), dict(iters=9),
                dict(delta_max=0.0), dict(delta_max=-0.1), dict(delta_max=nan), dict(axes=(1, 1))):
        with pytest.raises(ValueError):
            ofk.keyframe_rotation_setting(**bad)
    with pytest.raises(TypeError):
        ofk.keyframe_rotation_setting(sigma=3)


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
    for cfg in (PipelineConfig(), PipelineConfig.node(), PipelineConfig.baseline_1080p(), PipelineConfig(keyframe=True)):
        assert cfg.keyframe_rotation is None and cfg.keyframe_rotation_setting() is None
    assert PipelineConfig(keyframe=True, keyframe_rotation=False).keyframe_rotation_setting() is None
    assert PipelineConfig(keyframe_rotation=ofk.keyframe_rotation_setting(False)).keyframe_rotation_setting() is None
    on = PipelineConfig(track_table=True, keyframe=True, keyframe_rotation=ofk.keyframe_rotation_setting(sigma_bias=1e-3, iters=3))
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params())
    assert values(on.keyframe_rotation_setting()) == [1, 0, [1, 1, 1], 0.0, 1e-3, 1e-3, 3, 0.1]
    assert values(PipelineConfig(keyframe=True, keyframe_rotation=True).keyframe_rotation_setting()) == [1] + DEFAULTS
    with pytest.raises(ValueError):
        PipelineConfig(keyframe=True, keyframe_rotation="on").keyframe_rotation_setting()
    with pytest.raises(ValueError):                                # it refines the keyframe's rotation: no keyframe, nothing to refine
        PipelineConfig(keyframe_rotation=True).keyframe_rotation_setting()
    with pytest.raises(ValueError):
        PipelineConfig(keyframe=True, keyframe_rotation=make(ofk, [1, 0, [1, 1, 1], 0.0, 1e-4, 1e-3, 0, 0.1])).keyframe_rotation_setting()
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    Recorder.calls = []
    s = FlowStream(64, 48, batch=1, cfg=PipelineConfig(track_table=True, keyframe=True))
    assert not [c for c in Recorder.calls if c[0] == "set_keyframe_rotation"] and callable(s.key_rotation)
    FlowStream(64, 48, batch=1, cfg=on)
    names = [c[0] for c in Recorder.calls]
    sets = [c for c in Recorder.calls if c[0] == "set_keyframe_rotation"]
    assert len(sets) == 1 and values(sets[0][1][0]) == [1, 0, [1, 1, 1], 0.0, 1e-3, 1e-3, 3, 0.1]
    assert names.index("set_keyframe") < names.index("set_keyframe_rotation")       # one settings path, the keyframe first


def test_optical_fusion_hands_the_setting_to_its_pipeline_config(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    from of_amd.velocity_node import optical_fusion
    plain = optical_fusion(spin=False, keyframe=True)
    assert plain._keyframe_rotation == {} and plain.last_keyframe_rotation is None
    node = optical_fusion(spin=False, keyframe=True, keyframe_rotation=dict(sigma_bias=1e-3, source="attitude"))
    assert values(PipelineConfig(**node._keyframe, **node._keyframe_rotation).keyframe_rotation_setting()) == [1, 1, [1, 1, 1], 0.0, 1e-3, 1e-3, 2, 0.1]
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, keyframe=True, keyframe_rotation=dict(iters=0))
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, keyframe_rotation=True)       # without the keyframe
    from of_amd import simulation, velocity_node
    assert callable(simulation.keyframe_rotation_step) and callable(velocity_node.keyframe_rotation_step)


@pytest.mark.gpu
def test_setting_round_trip_and_every_refusal_leaves_it_as_it_was(pkg, ofk):
    ctx = ofk.Context(0, 64, 48, 2, 100, 2)
    try:
        assert values(ctx.get_keyframe_rotation()) == [0] + DEFAULTS     # off, the defaults behind it
        good = [1, 1, [1, 0, 1], 1e-5, 2e-4, 3e-3, 3, 0.05]
        ctx.set_keyframe_rotation(make(ofk, good))
        assert values(ctx.get_keyframe_rotation()) == good
        nan, inf = float("nan"), float("inf")
        for bad in (dict(mode=2), dict(mode=-1), dict(source=2), dict(source=-1), dict(sigma_gyro=-1e-9), dict(sigma_gyro=nan), dict(sigma_bias=-1.0),
                    dict(sigma_bias=nan), dict(sigma_att=-1.0), dict(sigma_att=nan), dict(sigma_att=inf), dict(iters=0), dict(iters=-1), dict(iters=9),
                    dict(delta_max=0.0), dict(delta_max=-0.1), dict(delta_max=nan)):
            with pytest.raises(ofk.OfkError) as e:
                ctx.set_keyframe_rotation(make(ofk, [dict(zip(NAMES, good), **bad)[n] for n in NAMES]))
            assert e.value.code == ofk.E_INVALID, bad
            assert values(ctx.get_keyframe_rotation()) == good, bad      # the previous setting is in place
        ctx.set_keyframe_rotation(make(ofk, [1, 0, [1, 1, 1], inf, inf, 0.0, 8, 1.0]))       # free axes are a setting
        ctx.set_keyframe_rotation(make(ofk, good))
        ctx.set_keyframe_rotation(None)
        assert ctx.get_keyframe_rotation().mode == 0 and values(ctx.get_keyframe_rotation())[1:] == good[1:]
        ctx.set_keyframe_rotation(iters=4)
        ctx.set_keyframe_rotation(make(ofk, [0, 7, [9, 9, 9], -9.0, -9.0, -9.0, -9, -9.0]))       # mode off: off, whatever else it holds
        assert ctx.get_keyframe_rotation().mode == 0 and ctx.get_keyframe_rotation().iters == 4
        with pytest.raises(ofk.OfkError):                          # nothing has stepped with the setting on
            ctx.keyframe_rotation_download(2)
    finally:
        ctx.close()
