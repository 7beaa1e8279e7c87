"""CPU-only: the track-gate entry points exist in the header, the binding and the library; k_track_gate is in the code object; the
pipeline configuration and the node carry the setting with defaults that mean "off"; track_gate_setting rejects bad keywords."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_track_gate", "ofk_get_track_gate", "ofk_track_gate_download", "ofk_lk_pyr_fb")


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
    for name, val in (("OFK_FB_OFF", 0), ("OFK_FB_PLAIN", 1), ("OFK_FB_SEEDED", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
    assert (ofk.FB_OFF, ofk.FB_PLAIN, ofk.FB_SEEDED) == (0, 1, 2)
    assert ofk.FB_MODES == {"off": 0, "plain": 1, "seeded": 2}
    m = re.search(r"typedef struct ofk_track_gate \{(.*?)\} ofk_track_gate;", txt, flags=re.S)
    assert m and re.findall(r"\b(int|double)\s+(\w+);", m.group(1)) == [("int", "fb_mode"), ("double", "fb_thr"), ("int", "fb_level"), ("double", "err_max")]
    assert [(n, t) for n, t in ofk.TrackGate._fields_] == [("fb_mode", C.c_int), ("fb_thr", C.c_double), ("fb_level", C.c_int), ("err_max", C.c_double)]
    assert len(lib.ofk_lk_pyr_fb.argtypes) == len(lib.ofk_lk_pyr_ex.argtypes) + 4


def test_gate_kernel_is_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    assert b"k_track_gate" in blob


def test_defaults_mean_off(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    for cfg in (PipelineConfig(), PipelineConfig.node(), PipelineConfig.of_module(), PipelineConfig.evaluate_exp(), PipelineConfig.baseline_1080p()):
        assert (cfg.fb_check, cfg.fb_thr, cfg.fb_level, cfg.err_max) == ("off", 0.5, -1, 0.0)
        assert cfg.track_gate_setting() is None
    g = PipelineConfig(fb_check="seeded", fb_thr=0.75, fb_level=0, err_max=12.5).track_gate_setting()
    assert (g.fb_mode, g.fb_thr, g.fb_level, g.err_max) == (ofk.FB_SEEDED, 0.75, 0, 12.5)
    g = PipelineConfig(err_max=3.0).track_gate_setting()        # the err cap alone is a gate too
    assert (g.fb_mode, g.err_max) == (ofk.FB_OFF, 3.0)
    d = ofk.track_gate_setting()
    assert (d.fb_mode, d.fb_thr, d.fb_level, d.err_max) == (ofk.FB_OFF, 0.5, -1, 0.0)
    import inspect
    from of_amd import velocity_node
    assert inspect.signature(velocity_node.optical_fusion.__init__).parameters["track_gate"].default is None
    assert velocity_node.optical_fusion._track_gate == {}


@pytest.mark.parametrize("kw", [dict(fb="sideways"), dict(fb=3), dict(fb="plain", fb_thr=0.0), dict(fb="seeded", fb_thr=-1.0),
                                dict(fb="plain", fb_thr=float("nan")), dict(fb="plain", fb_thr=float("inf")), dict(fb_level=-2),
                                dict(err_max=-0.5), dict(err_max=float("nan")), dict(err_max=float("inf"))])
def test_track_gate_setting_rejects_bad_keywords(built, ofk, kw):
    with pytest.raises(ValueError):
        ofk.track_gate_setting(**kw)


def test_track_gate_setting_takes_names_and_numbers(built, ofk):
    assert ofk.track_gate_setting("plain").fb_mode == ofk.track_gate_setting(ofk.FB_PLAIN).fb_mode == 1
    assert ofk.track_gate_setting("off", fb_thr=-1.0).fb_mode == 0       # the threshold only matters with the check on
    with pytest.raises(TypeError):
        ofk.track_gate_setting(threshold=1.0)
