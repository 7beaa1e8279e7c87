"""The perspective warp's entry point exists in the header, the binding and the library; its constants agree on both sides; the kernel
is in the code object in both channel counts; the facade refuses what is out of scope before it asks for a device (CPU-only)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONSTANTS = (("OFK_BORDER_CONSTANT", 0), ("OFK_BORDER_REPLICATE", 1))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge


def test_entry_point_declared_bound_and_exported(built, ofk):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofk.h")).read(), flags=re.S)
    lib = ofk.load_library()
    s = "ofk_warp_perspective"
    m = re.search(r"int %s\s*\((.*?)\);" % s, txt, flags=re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == \
        "ofk_ctx *ctx, const uint8_t *src, int sh, int sw, int channels, const double *M, uint8_t *dst, int dh, int dw, " \
        "int border, int border_value, int batch, int *covered"
    assert s in ofk.SYMBOLS and hasattr(lib, s) and len(getattr(lib, s).argtypes) == 13
    for name, val in CONSTANTS:
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
        assert getattr(ofk, name[4:]) == val, name
    assert ofk.BORDERS == {"constant": 0, "replicate": 1}
    assert lib.ofk_warp_perspective(None, None, 1, 1, 1, None, None, 1, 1, 0, 0, 1, None) == ofk.E_INVALID
    assert callable(ofk.Context.warp_perspective)


def test_warp_kernel_is_in_the_code_object_for_both_channel_counts(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for k in (b"k_warp_u8ILi1E", b"k_warp_u8ILi3E"):
        assert k in blob, k
    mk = open(os.path.join(os.path.dirname(ofk.LIB_PATH), "csrc", "Makefile")).read()
    assert re.search(r"^build/k_image\.o:.*\bk_warp\.inc\b", mk, flags=re.M)


def test_facade_constants_and_refusals(built, pkg):
    from of_amd import cv2_hip
    assert (cv2_hip.INTER_NEAREST, cv2_hip.INTER_LINEAR, cv2_hip.INTER_CUBIC, cv2_hip.WARP_INVERSE_MAP) == (0, 1, 2, 16)
    assert (cv2_hip.BORDER_CONSTANT, cv2_hip.BORDER_REPLICATE) == (0, 1)
    img, M = np.zeros((8, 8), np.uint8), np.eye(3)
    for flags in (cv2_hip.INTER_NEAREST, cv2_hip.INTER_CUBIC, cv2_hip.INTER_CUBIC | cv2_hip.WARP_INVERSE_MAP, cv2_hip.INTER_AREA, cv2_hip.INTER_LANCZOS4):
        with pytest.raises(NotImplementedError):
            cv2_hip.warpPerspective(img, M, (8, 8), flags=flags)
    with pytest.raises(NotImplementedError):
        cv2_hip.warpPerspective(img, M, (8, 8), borderMode=4)       # BORDER_REFLECT_101
    with pytest.raises(NotImplementedError):
        cv2_hip.warpPerspective(np.zeros((8, 8, 3), np.uint8), M, (8, 8), borderValue=(1, 2, 3))
    with pytest.raises(NotImplementedError):
        cv2_hip.warpPerspective(img, M, (8, 8), borderValue=300)
    for bad in (np.zeros((8, 8), np.float32), np.zeros((8, 8, 2), np.uint8), np.zeros((8,), np.uint8)):
        with pytest.raises(ValueError):
            cv2_hip.warpPerspective(bad, M, (8, 8))
    with pytest.raises(ValueError):
        cv2_hip.warpPerspective(img, np.eye(2), (8, 8))
    with pytest.raises(ValueError):
        cv2_hip.warpPerspective(img, np.zeros((3, 3)), (8, 8))      # singular: no inverse to warp through


# ------------------------------------------------------------------------------------------------ the view per stream
NEW = ("ofk_set_stabilise", "ofk_get_stabilise", "ofk_stab_download", "ofk_stab_frames", "ofk_stab_reset", "ofk_stab_pose")
NAMES = ["mode", "border", "border_value", "min_cover", "chain"]
DEFAULTS = [0, 0, 0.5, 1]                                        # behind the mode
STAB_CONSTANTS = (("OFK_STAB_OFF", 0), ("OFK_STAB_ROTATION", 1), ("OFK_STAB_PLANE", 2), ("OFK_STAB_DOUBLES", 48), ("OFK_STAB_INTS", 4), ("OFK_STAB_NONE", 0),
                  ("OFK_STAB_ROTATION_ONLY", 1), ("OFK_STAB_FULL", 2), ("OFK_STAB_RB_COVER", 1), ("OFK_STAB_RB_FINITE", 2))


def values(s):
    return [getattr(s, n) for n in NAMES]


def test_view_entry_points_declared_bound_and_exported(built, ofk):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofk.h")).read(), flags=re.S)
    lib = ofk.load_library()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert s in ofk.SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
    for name, val in STAB_CONSTANTS:
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
        assert getattr(ofk, name[4:]) == val, name
    m = re.search(r"typedef struct ofk_stabilise \{(.*?)\} ofk_stabilise;", txt, flags=re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "int mode; int border; int border_value; double min_cover; int chain;"
    want = [("mode", C.c_int), ("border", C.c_int), ("border_value", C.c_int), ("min_cover", C.c_double), ("chain", C.c_int)]
    assert list(ofk.Stabilise._fields_) == want and C.sizeof(ofk.Stabilise) == 32
    assert [getattr(ofk.Stabilise, n).offset for n in NAMES] == [0, 4, 8, 16, 24]
    assert ("stabilise", ofk.Stabilise) in ofk.SETTINGS
    assert len(lib.ofk_stab_download.argtypes) == 4 and len(lib.ofk_stab_pose.argtypes) == 13
    assert lib.ofk_set_stabilise(None, None) == ofk.E_INVALID and lib.ofk_get_stabilise(None, None) == ofk.E_INVALID
    assert lib.ofk_stab_download(None, None, None, None) == ofk.E_INVALID and lib.ofk_stab_reset(None, 0) == ofk.E_INVALID
    assert lib.ofk_stab_frames(None, None, None) == ofk.E_INVALID
    assert lib.ofk_stab_pose(None, None, None, None, None, None, None, 1, 1, None, None, 1, None) == ofk.E_INVALID


def test_view_kernels_are_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for k in (b"k_stab_pose", b"k_stab_clear", b"k_keyframe_step"):
        assert k in blob, k
    mk = open(os.path.join(os.path.dirname(ofk.LIB_PATH), "csrc", "Makefile")).read()
    assert re.search(r"^build/k_tracks\.o:.*\bk_stabilise\.inc\b", mk, flags=re.M)


def test_view_settings_from_names(built, ofk):
    assert values(ofk.stabilise_setting()) == [2] + DEFAULTS
    m = ofk.stabilise_setting("rotation", border="replicate", border_value=200, min_cover=0.0, chain=0)
    assert values(m) == [1, 1, 200, 0.0, 0]
    assert ofk.stabilise_setting("plane").mode == 2 and ofk.stabilise_setting(ofk.STAB_ROTATION).mode == 1
    assert ofk.stabilise_setting(False, min_cover=7.0).mode == 0     # off: the other fields are not looked at
    nan, inf = float("nan"), float("inf")
    for bad in (dict(mode=3), dict(mode=-1), dict(border=2), dict(border_value=256), dict(border_value=-1), dict(min_cover=1.0), dict(min_cover=-0.1),
                dict(min_cover=nan), dict(min_cover=inf), dict(chain=2), dict(chain=-1)):
        with pytest.raises(ValueError):
            ofk.stabilise_setting(**bad)
    with pytest.raises(TypeError):
        ofk.stabilise_setting(sigma=3)


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
    from of_amd.pipeline import CameraModel, FlowStream, PipelineConfig, RollingShutter
    for cfg in (PipelineConfig(), PipelineConfig.node(), PipelineConfig.baseline_1080p(), PipelineConfig(track_table=True, keyframe=True)):
        assert cfg.stabilise is None and cfg.stabilise_setting() is None
    assert PipelineConfig(track_table=True, keyframe=True, stabilise=False).stabilise_setting() is None
    assert PipelineConfig(stabilise=ofk.stabilise_setting(False)).stabilise_setting() is None
    on = PipelineConfig(track_table=True, keyframe=True, stabilise=ofk.stabilise_setting("rotation", min_cover=0.7))
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params())
    assert values(on.stabilise_setting()) == [1, 0, 0, 0.7, 1]
    assert values(PipelineConfig(track_table=True, keyframe=True, stabilise=True).stabilise_setting()) == [2] + DEFAULTS
    with pytest.raises(ValueError):
        PipelineConfig(keyframe=True, stabilise="on").stabilise_setting()
    with pytest.raises(ValueError):                                # the view is the keyframe's
        PipelineConfig(track_table=True, stabilise=True).stabilise_setting()
    with pytest.raises(ValueError):                                # a raw frame behind a lens needs a remap in front
        PipelineConfig(keyframe=True, stabilise=True, camera=CameraModel(fx=160.0, fy=160.0, cx=80.0, cy=64.0, k=(-0.1, 0.01, 0, 0))).stabilise_setting()
    with pytest.raises(ValueError):
        PipelineConfig(keyframe=True, stabilise=True, rolling_shutter=RollingShutter(mode="flow", readout=0.5)).stabilise_setting()
    with pytest.raises(ValueError):
        PipelineConfig(keyframe=True, stabilise=ofk.Stabilise(2, 0, 0, 1.5, 1)).stabilise_setting()
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    Recorder.calls = []
    s = FlowStream(64, 48, batch=1, cfg=PipelineConfig(track_table=True, keyframe=True))
    assert not [c for c in Recorder.calls if c[0] == "set_stabilise"] and callable(s.stabilised)
    FlowStream(64, 48, batch=1, cfg=on)
    names = [c[0] for c in Recorder.calls]
    sets = [c for c in Recorder.calls if c[0] == "set_stabilise"]
    assert len(sets) == 1 and values(sets[0][1][0]) == [1, 0, 0, 0.7, 1]
    assert names.index("set_keyframe") < names.index("set_stabilise")
    Recorder.calls = []                                            # independent pairs have no keyframe: FlowPipeline ignores the setting
    pipeline.FlowPipeline(64, 48, batch=1, cfg=on)
    assert not [c for c in Recorder.calls if c[0] == "set_stabilise"]


def test_optical_fusion_hands_the_setting_to_its_pipeline_config(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    from of_amd.velocity_node import optical_fusion
    plain = optical_fusion(spin=False, keyframe=True)
    assert plain._stabilise == {} and plain.last_stabilised is None
    node = optical_fusion(spin=False, stabilise=dict(mode="rotation", min_cover=0.7))      # it switches the keyframe and the table on
    assert node._keyframe and node._track_table
    cfg = PipelineConfig(**node._track_table, **node._keyframe, **node._stabilise)
    assert values(cfg.stabilise_setting()) == [1, 0, 0, 0.7, 1]
    assert values(PipelineConfig(**{**optical_fusion(spin=False, stabilise=True)._stabilise, "keyframe": True}).stabilise_setting()) == [2] + DEFAULTS
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, stabilise=dict(min_cover=2.0))
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, stabilise=True, camera=dict(fx=160.0, fy=160.0, cx=80.0, cy=64.0, k=(-0.1, 0.01, 0, 0)))
    from of_amd import simulation, velocity_node
    assert callable(simulation.stabilise_step) and callable(velocity_node.stabilise_step)


@pytest.mark.gpu
def test_setting_round_trip_and_every_refusal_leaves_it_as_it_was(pkg, ofk):
    ctx = ofk.Context(0, 64, 48, 2, 100, 2)
    try:
        assert values(ctx.get_stabilise()) == [0] + DEFAULTS       # off, the defaults behind it
        good = [1, 1, 200, 0.25, 0]
        ctx.set_stabilise(ofk.Stabilise(*good))
        assert values(ctx.get_stabilise()) == good
        nan, inf = float("nan"), float("inf")
        for bad in (dict(mode=3), dict(mode=-1), dict(border=2), dict(border=-1), dict(border_value=256), dict(border_value=-1), dict(min_cover=1.0),
                    dict(min_cover=-0.1), dict(min_cover=nan), dict(min_cover=inf), dict(chain=2), dict(chain=-1)):
            with pytest.raises(ofk.OfkError) as e:
                ctx.set_stabilise(ofk.Stabilise(*[dict(zip(NAMES, good), **bad)[n] for n in NAMES]))
            assert e.value.code == ofk.E_INVALID, bad
            assert values(ctx.get_stabilise()) == good, bad        # the previous setting is in place
        ctx.set_stabilise(None)
        assert ctx.get_stabilise().mode == 0 and values(ctx.get_stabilise())[1:] == good[1:]
        ctx.set_stabilise(min_cover=0.75)
        ctx.set_stabilise(ofk.Stabilise(0, -9, -9, -9.0, -9))      # mode off: off, whatever else it holds
        assert ctx.get_stabilise().mode == 0 and ctx.get_stabilise().min_cover == 0.75
        with pytest.raises(ofk.OfkError):                          # nothing has stepped with the setting on
            ctx.stab_download(2, 48, 64)
    finally:
        ctx.close()
