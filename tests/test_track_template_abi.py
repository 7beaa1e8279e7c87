"""The track-template entry points exist in the header, the binding and the library; the setting's structure agrees on both sides; the
kernels are in the code object; the pipeline configuration carries the setting with a default that means "off" and only streams apply
it; optical_fusion hands it down (CPU-only).  On a device: the setting's defaults, its round trip, every invalid field, "off" after
NULL, and a stream step with the setting on and the track table off."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_track_template", "ofk_get_track_template", "ofk_track_template_download", "ofk_track_affine_fit", "ofk_track_template_step")
FIELDS = [("mode", "int"), ("win", "int"), ("ncc_min", "double"), ("anchor_iters", "int"), ("anchor_max", "double"), ("outside", "int"),
          ("fit_min", "int"), ("fit_gate", "double"), ("scale_max", "double")]
NAMES = [n for n, _ in FIELDS]
DEFAULTS = [15, 0.8, 3, 2.0, 0, 6, 2.0, 1.5]                     # behind the mode
CONSTANTS = (("OFK_TPL_OFF", 0), ("OFK_TPL_ON", 1), ("OFK_TPL_DOUBLES", 32), ("OFK_TPL_KEEP", 0), ("OFK_TPL_DROP", 1), ("OFK_TPL_NOT_TRACKED", 0),
             ("OFK_TPL_PASS", 1), ("OFK_TPL_FAIL", 2), ("OFK_TPL_ABANDONED", 3), ("OFK_TPL_OUTSIDE", 4), ("OFK_TPL_FLAT", 5),
             ("OFK_TPL_NO_TEMPLATE", 6), ("OFK_TPL_CAPTURED", 16))


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
    assert (ofk.TPL_OFF, ofk.TPL_ON, ofk.TPL_DOUBLES, ofk.TPL_KEEP, ofk.TPL_DROP) == (0, 1, 32, 0, 1)
    assert (ofk.TPL_NOT_TRACKED, ofk.TPL_PASS, ofk.TPL_FAIL, ofk.TPL_ABANDONED, ofk.TPL_OUTSIDE_ROW, ofk.TPL_FLAT, ofk.TPL_NO_TEMPLATE,
            ofk.TPL_CAPTURED) == (0, 1, 2, 3, 4, 5, 6, 16)
    m = re.search(r"typedef struct ofk_track_template \{(.*?)\} ofk_track_template;", txt, flags=re.S)
    assert m and re.findall(r"\b(int|double)\s+(\w+);", m.group(1)) == [(t, n) for n, t in FIELDS]
    ctype = {"int": C.c_int, "double": C.c_double}
    assert [(n, t) for n, t in ofk.TrackTemplate._fields_] == [(n, ctype[t]) for n, t in FIELDS] and C.sizeof(ofk.TrackTemplate) == 56
    assert [getattr(ofk.TrackTemplate, n).offset for n in NAMES] == [0, 4, 8, 16, 24, 32, 36, 40, 48]
    assert ("track_template", ofk.TrackTemplate) in ofk.SETTINGS
    assert len(lib.ofk_track_template_download.argtypes) == 8 and len(lib.ofk_track_affine_fit.argtypes) == 12
    assert len(lib.ofk_track_template_step.argtypes) == 22
    assert lib.ofk_set_track_template(None, None) == ofk.E_INVALID and lib.ofk_get_track_template(None, None) == ofk.E_INVALID
    assert lib.ofk_track_template_download(None, None, None, None, None, None, 1, None) == ofk.E_INVALID
    assert lib.ofk_track_affine_fit(None, None, None, None, None, None, 1, 1, 8, 8, None, None) == ofk.E_INVALID
    assert [ofk.tpl_stride(w) for w in (5, 15, 21, 31)] == [52, 292, 532, 1092]


def test_template_kernels_are_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    # the mangled names, length first and the first argument behind them: k_track_template is no prefix match of k_track_template_update
    for k in (rb"_Z14k_track_affineP", rb"_Z16k_track_template\d", rb"_Z23k_track_template_update\d"):
        assert re.search(k, blob), k
    assert not re.search(rb"_Z16k_track_template\d", b"_Z23k_track_template_update8tp_state")


def test_settings_from_names(built, ofk):
    assert values(ofk.track_template_setting()) == [1] + DEFAULTS
    t = ofk.track_template_setting(win=21, ncc_min=-1.0, anchor_iters=0, anchor_max=0.5, outside="drop", fit_min=3, fit_gate=0.0, scale_max=0.0)
    assert values(t) == [1, 21, -1.0, 0, 0.5, 1, 3, 0.0, 0.0]
    assert ofk.track_template_setting(outside=ofk.TPL_DROP).outside == 1
    assert ofk.track_template_setting(False, win=4).mode == 0                  # off: the other fields are not looked at
    nan, inf = float("nan"), float("inf")
    for bad in (dict(mode=2), dict(win=4), dict(win=3), dict(win=33), dict(win=16), dict(ncc_min=-1.01), dict(ncc_min=1.5), dict(ncc_min=nan),
                dict(anchor_iters=-1), dict(anchor_iters=9), dict(anchor_max=0.0), dict(anchor_max=-1.0), dict(anchor_max=inf), dict(outside=2),
                dict(outside="lose"), dict(fit_min=2), dict(fit_gate=-0.5), dict(fit_gate=nan), dict(scale_max=0.5), dict(scale_max=-2.0),
                dict(scale_max=inf), dict(scale_max=nan)):
        with pytest.raises(ValueError):
            ofk.track_template_setting(**bad)
    with pytest.raises(TypeError):
        ofk.track_template_setting(window=15)


class Recorder:
    """Stands in for ofk.Context: records what a pipeline applies to it."""
    calls = []

    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        def f(*a, **k):
            Recorder.calls.append((name, a, k))
        return f


def test_pipeline_config_default_means_off_and_only_streams_apply_it(built, pkg, ofk, monkeypatch):
    from of_amd import pipeline
    from of_amd.pipeline import PipelineConfig, FlowPipeline, FlowStream
    for cfg in (PipelineConfig(), PipelineConfig.node(), PipelineConfig.of_module(), PipelineConfig.evaluate_exp(), PipelineConfig.baseline_1080p()):
        assert cfg.track_template is None and cfg.track_template_setting() is None
    assert PipelineConfig(track_template=False).track_template_setting() is None
    assert PipelineConfig(track_template=ofk.track_template_setting(False)).track_template_setting() is None
    on = PipelineConfig(track_table=True, track_template=ofk.track_template_setting(ncc_min=0.9, anchor_iters=0))
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params())          # to_params() does not know the setting
    assert values(on.track_template_setting()) == [1, 15, 0.9, 0, 2.0, 0, 6, 2.0, 1.5]
    assert values(PipelineConfig(track_template=True).track_template_setting()) == [1] + DEFAULTS
    with pytest.raises(ValueError):
        PipelineConfig(track_template="on").track_template_setting()
    with pytest.raises(ValueError):
        PipelineConfig(track_template=ofk.TrackTemplate(1, 16, 0.8, 3, 2.0, 0, 6, 2.0, 1.5)).track_template_setting()
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    Recorder.calls = []
    s = FlowStream(64, 48, batch=1, cfg=PipelineConfig())
    FlowPipeline(64, 48, batch=1, cfg=on)                        # frame pairs ignore the setting
    assert not [c for c in Recorder.calls if c[0] == "set_track_template"] and callable(s.templates)
    FlowStream(64, 48, batch=1, cfg=on)
    names = [c[0] for c in Recorder.calls]
    sets = [c for c in Recorder.calls if c[0] == "set_track_template"]
    assert len(sets) == 1 and values(sets[0][1][0]) == [1, 15, 0.9, 0, 2.0, 0, 6, 2.0, 1.5]
    assert names.index("set_track_table") < names.index("set_track_template")     # one settings path, the table first


def test_optical_fusion_hands_the_template_setting_to_its_pipeline_config(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    from of_amd.velocity_node import optical_fusion
    plain = optical_fusion(spin=False)
    assert plain._track_template == {} and plain._track_table == {} and plain.last_track_template is None
    node = optical_fusion(spin=False, track_template=dict(ncc_min=0.9, outside="drop"))
    assert values(PipelineConfig(**node._track_template).track_template_setting()) == [1, 15, 0.9, 3, 2.0, 1, 6, 2.0, 1.5]
    assert node._track_table == dict(track_table=True)           # the templates need the table
    both = optical_fusion(spin=False, track_template=True, track_table=dict(seed="flow"))
    assert both._track_template == dict(track_template=True) and both._track_table["track_table"].seed == ofk.TT_SEED_FLOW
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, track_template=dict(win=16))
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, track_template=dict(window=15))
    from of_amd import velocity_node
    assert callable(velocity_node.track_template_step)


@pytest.mark.gpu
def test_setting_round_trip_invalid_fields_off_after_null_and_the_table(pkg, ofk):
    ctx = ofk.Context(0, 64, 48, 2, 100, 2)
    try:
        assert values(ctx.get_track_template()) == [0] + DEFAULTS   # off, the defaults behind it
        ctx.set_track_template(win=21, ncc_min=0.5, anchor_iters=8, anchor_max=1.0, outside="drop", fit_min=3, fit_gate=0.0, scale_max=0.0)
        good = [1, 21, 0.5, 8, 1.0, 1, 3, 0.0, 0.0]
        assert values(ctx.get_track_template()) == good
        nan, inf = float("nan"), float("inf")
        for bad in (dict(mode=2), dict(mode=-1), dict(win=3), dict(win=33), dict(win=20), dict(ncc_min=-1.5), dict(ncc_min=1.01), dict(ncc_min=nan),
                    dict(ncc_min=inf), dict(anchor_iters=-1), dict(anchor_iters=9), dict(anchor_max=0.0), dict(anchor_max=-2.0), dict(anchor_max=nan),
                    dict(anchor_max=inf), dict(outside=2), dict(outside=-1), dict(fit_min=2), dict(fit_min=0), dict(fit_gate=-1e-9), dict(fit_gate=nan),
                    dict(fit_gate=inf), dict(scale_max=0.99), dict(scale_max=-1.0), dict(scale_max=nan), dict(scale_max=inf)):
            with pytest.raises(ofk.OfkError) as e:
                ctx.set_track_template(ofk.TrackTemplate(*[dict(zip(NAMES, good), **bad)[n] for n in NAMES]))
            assert e.value.code == ofk.E_INVALID, bad
            assert values(ctx.get_track_template()) == good, bad    # the previous setting is in place
        ctx.set_track_template(None)
        assert ctx.get_track_template().mode == 0 and values(ctx.get_track_template())[1:] == good[1:]
        ctx.set_track_template(ncc_min=0.7)
        ctx.set_track_template(ofk.TrackTemplate(0, -9, -9.0, -9, -9.0, -9, -9, -9.0, -9.0))   # mode off: off, whatever else the structure holds
        assert ctx.get_track_template().mode == 0 and ctx.get_track_template().ncc_min == 0.7
        with pytest.raises(ofk.OfkError):                          # nothing has stepped with the setting on
            ctx.track_template_download(2)
        # a stream step with the setting on and the track table off is refused before any launch, and the stream goes on without it
        from of_amd import synth
        from of_amd.pipeline import PipelineConfig
        frames, info = synth.render_sequence(48, 64, 3, 3, margin=32)
        p = PipelineConfig(max_corners=100, quality=0.01, min_distance=4, block_size=3, win=15, max_level=2).to_params()
        sensors = ofk.make_sensors(1, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"], v_prior=info["v"])
        ctx.stream_begin(frames[None, 0], p)
        ctx.set_track_template(ofk.track_template_setting())
        with pytest.raises(ofk.OfkError) as e:
            ctx.stream_step(frames[None, 1], sensors, p, 10, 5)
        assert e.value.code == ofk.E_INVALID and "ofk_set_track_table" in str(e.value)
        ctx.set_track_table(ofk.track_table_setting())
        ctx.stream_step(frames[None, 1], sensors, p, 10, 5)
        assert ctx.track_template_download(1)["rec"][0, 16] > 0      # rows captured
        ctx.set_track_template(None)
        ctx.stream_step(frames[None, 2], sensors, p, 10, 5)
    finally:
        ctx.close()
