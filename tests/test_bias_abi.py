"""The gyro bias's entry points exist in the header, the binding and the library; the setting's structure has the C ABI's layout; the
pipeline configuration carries the setting with a default that means "off" and only the streams apply it; optical_fusion hands it
down; the setter's refusals, which need no device (a context does: those run on the GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_gyro_bias", "ofk_get_gyro_bias", "ofk_gyro_bias_reset", "ofk_gyro_bias_download", "ofk_gyro_bias_step")


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
    for name, val in (("OFK_BIAS_OFF", 0), ("OFK_BIAS_ON", 1), ("OFK_BIAS_DOUBLES", 32)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
    assert (ofk.BIAS_OFF, ofk.BIAS_ON, ofk.BIAS_DOUBLES) == (0, 1, 32)
    m = re.search(r"typedef struct ofk_gyro_bias \{([^}]*)\} ofk_gyro_bias;", txt)
    assert m
    names = [re.sub(r"\[\d+\]", "", n.strip().split()[-1]) for f in m.group(1).split(";") if f.strip() for n in f.split(",")]
    assert names == [n for n, _ in ofk.GyroBias._fields_] == ["mode", "sigma_flow", "sigma_gyro", "q", "p0", "b0", "nis_max", "update"]
    # int, 10 doubles (p0[3] and b0[3] among them), int under the C ABI's alignment: 8 + 80 + 8
    G = ofk.GyroBias
    assert C.sizeof(G) == 96
    assert (G.sigma_flow.offset, G.sigma_gyro.offset, G.q.offset, G.p0.offset, G.b0.offset, G.nis_max.offset, G.update.offset) == (8, 16, 24, 32, 56, 80, 88)
    assert ("gyro_bias", G) in ofk.SETTINGS


def test_bias_kernels_are_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for k in (b"k_gyro_bias_apply", b"k_stream_bias", b"k_bias_solve", b"k_stream_joint", b"k_stream_fuse"):
        assert k in blob, k


def test_settings_from_names(built, ofk):
    g = ofk.gyro_bias_setting()
    assert (g.mode, g.sigma_flow, g.sigma_gyro, g.q, list(g.p0), list(g.b0), g.nis_max, g.update) == (1, 0.2, 0.0, 1e-12, [1e-2] * 3, [0.0] * 3, 0.0, 1)
    g = ofk.gyro_bias_setting(True, 0.3, 2e-5, 1e-10, (0.0, 1e-3, 1e-2), (1e-3, -1e-3, 0.0), 16.0, update=False)
    assert (g.sigma_flow, g.sigma_gyro, g.q, list(g.p0), list(g.b0), g.nis_max, g.update) == (0.3, 2e-5, 1e-10, [0.0, 1e-3, 1e-2], [1e-3, -1e-3, 0.0], 16.0, 0)
    assert ofk.gyro_bias_setting(False).mode == 0


def test_the_setter_refuses_without_a_device(built, ofk):
    """ofk_set_gyro_bias / ofk_get_gyro_bias / the downloads with no context: OFK_E_INVALID, nothing is touched."""
    lib = ofk.load_library()
    g = ofk.gyro_bias_setting()
    assert lib.ofk_set_gyro_bias(None, C.byref(g)) == ofk.E_INVALID
    assert lib.ofk_get_gyro_bias(None, C.byref(g)) == ofk.E_INVALID
    assert lib.ofk_gyro_bias_download(None, None) == ofk.E_INVALID
    assert lib.ofk_gyro_bias_reset(None, None, 1) == ofk.E_INVALID
    assert lib.ofk_gyro_bias_step(None, 0, None, None, None, 1, 1, None, None, None, None, None, None, None, None) == ofk.E_INVALID


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
        assert cfg.gyro_bias is None and cfg.gyro_bias_setting() is None
    assert PipelineConfig(gyro_bias=False).gyro_bias_setting() is None
    assert PipelineConfig(gyro_bias=ofk.gyro_bias_setting(False)).gyro_bias_setting() is None
    on = PipelineConfig(gyro_bias=ofk.gyro_bias_setting(sigma_gyro=2e-5))
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params())         # to_params() does not know the setting
    assert on.gyro_bias_setting().sigma_gyro == 2e-5 and PipelineConfig(gyro_bias=True).gyro_bias_setting().mode == 1
    with pytest.raises(ValueError):
        PipelineConfig(gyro_bias=dict(q=1.0)).gyro_bias_setting()
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    Recorder.calls = []
    fs = FlowStream(64, 48, batch=1, cfg=PipelineConfig())
    assert not [c for c in Recorder.calls if c[0] == "set_gyro_bias"] and hasattr(fs, "gyro_bias")
    FlowStream(64, 48, batch=1, cfg=on)
    sets = [c for c in Recorder.calls if c[0] == "set_gyro_bias"]
    assert len(sets) == 1 and sets[0][1][0].sigma_gyro == 2e-5
    Recorder.calls = []
    FlowPipeline(64, 48, batch=1, cfg=on)                                       # independent pairs carry no state
    assert not [c for c in Recorder.calls if c[0] == "set_gyro_bias"]


def test_optical_fusion_hands_the_setting_to_its_pipeline_config(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    from of_amd.velocity_node import optical_fusion, gyro_bias_step
    from of_amd import simulation
    assert optical_fusion(spin=False)._gyro_bias == {}
    node = optical_fusion(spin=False, gyro_bias=dict(sigma_gyro=2e-5, p0=(0.0, 1e-2, 1e-2)))
    g = PipelineConfig(**node._gyro_bias).gyro_bias_setting()
    assert (g.mode, g.sigma_gyro, list(g.p0)) == (1, 2e-5, [0.0, 1e-2, 1e-2]) and node.last_gyro_bias is None
    assert optical_fusion(spin=False, gyro_bias=True)._gyro_bias == dict(gyro_bias=True)
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, gyro_bias=dict(sigma_omega=1.0))
    assert callable(gyro_bias_step) and callable(simulation.gyro_bias_step)


def values(g):
    return [g.mode, g.sigma_flow, g.sigma_gyro, g.q, list(g.p0), list(g.b0), g.nis_max, g.update]


@pytest.mark.gpu
def test_setting_round_trip_every_refusal_and_off_after_null(pkg, ofk):
    ctx = ofk.Context(0, 64, 48, 2, 100, 2)
    try:
        assert ctx.get_gyro_bias().mode == 0                     # off
        good = dict(mode=1, sigma_flow=0.25, sigma_gyro=2e-5, q=1e-12, p0=(1e-2, 0.0, 1e-3), b0=(1e-3, -1e-3, 0.0), nis_max=16.0, update=1)

        def make(**over):
            d = dict(good, **over)
            return ofk.GyroBias(d["mode"], d["sigma_flow"], d["sigma_gyro"], d["q"], (C.c_double * 3)(*d["p0"]), (C.c_double * 3)(*d["b0"]),
                                d["nis_max"], d["update"])
        with pytest.raises(ofk.OfkError):                        # the setting is off: nothing to load a state into
            ctx.gyro_bias_reset(np.zeros((1, 9)))
        ctx.set_gyro_bias(make())
        assert values(ctx.get_gyro_bias()) == values(make())
        with pytest.raises(ofk.OfkError) as e:                   # no step with the setting on yet
            ctx.gyro_bias_download(1)
        assert e.value.code == ofk.E_INVALID
        nan, inf = float("nan"), float("inf")
        x = np.array([[0.5, 0.4], [-0.5, -0.4], [0.5, -0.4], [-0.3, 0.4]]); u = np.full((4, 2), 1e-3)
        kw = dict(d=1.0, nrm=(0.0, 0.0, 1.0), omega=(0.0, 0.0, 0.0))
        for bad in (dict(mode=2), dict(mode=-1), dict(sigma_flow=0.0), dict(sigma_flow=-0.1), dict(sigma_flow=nan), dict(sigma_flow=inf),
                    dict(sigma_gyro=-1e-5), dict(sigma_gyro=nan), dict(sigma_gyro=inf), dict(q=-1e-12), dict(q=nan), dict(q=inf),
                    dict(p0=(-1e-3, 0.0, 0.0)), dict(p0=(0.0, nan, 0.0)), dict(p0=(0.0, 0.0, inf)), dict(b0=(nan, 0.0, 0.0)), dict(b0=(0.0, -inf, 0.0)),
                    dict(nis_max=-1.0), dict(nis_max=nan), dict(update=2)):
            for call in (ctx.set_gyro_bias, lambda g: ctx.gyro_bias_step(ofk.SOLVE_NODE, x, u, gyro_bias=g, **kw)):
                with pytest.raises(ofk.OfkError) as e:
                    call(make(**bad))
                assert e.value.code == ofk.E_INVALID, bad
            assert values(ctx.get_gyro_bias()) == values(make()), bad                 # the previous setting is in place
        with pytest.raises(ofk.OfkError):                        # off is no mode for the stage entry
            ctx.gyro_bias_step(ofk.SOLVE_NODE, x, u, gyro_bias=make(mode=0), **kw)
        with pytest.raises(ofk.OfkError):                        # OFMODULE is not the sensor model
            ctx.gyro_bias_step(ofk.SOLVE_OFMODULE, x, u, gyro_bias=make(), **kw)
        for bad in (np.full((1, 9), nan), np.zeros((3, 9))):     # a state that is not finite; more streams than the context has
            with pytest.raises(ofk.OfkError):
                ctx.gyro_bias_reset(bad)
        out, st = ctx.gyro_bias_step(ofk.SOLVE_NODE, x, u, gyro_bias=make(), **kw)
        assert out.shape == (8,) and st.shape == (32,) and st[21] == 1
        assert values(ctx.get_gyro_bias()) == values(make())     # the stage entry touches no setting
        ctx.set_gyro_bias(make(sigma_flow=1e-300, sigma_gyro=0.0, q=0.0, p0=(0.0, 0.0, 0.0), nis_max=0.0, update=0))   # the ends of every range are inside
        ctx.set_gyro_bias(None)
        assert ctx.get_gyro_bias().mode == 0 and ctx.get_gyro_bias().sigma_flow == 1e-300
        ctx.set_gyro_bias(sigma_flow=0.5)
        assert values(ctx.get_gyro_bias())[:2] == [1, 0.5]
    finally:
        ctx.close()
