"""The epipolar solve's entry points exist in the header, the binding and the library; the setting's structure has the C ABI's size;
the pipeline configuration carries the setting with defaults that mean "off"; optical_fusion hands it down.  On the GPU (a context
needs one): get after set, every refusal rule, a refused setting leaves the previous one in place."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_epipolar", "ofk_get_epipolar", "ofk_epipolar_download", "ofk_epipolar_points_download", "ofk_velocity_solve_epipolar")


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
    for name, val in (("OFK_EPI_OFF", 0), ("OFK_EPI_ON", 1), ("OFK_EPI_W_ONE", 0), ("OFK_EPI_W_ROBUST", 1), ("OFK_EPI_DOUBLES", 32)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
    assert (ofk.EPI_OFF, ofk.EPI_ON, ofk.EPI_W_ONE, ofk.EPI_W_ROBUST, ofk.EPI_DOUBLES) == (0, 1, 0, 1, 32)
    m = re.search(r"typedef struct ofk_epipolar \{([^}]*)\} ofk_epipolar;", txt)
    assert m
    names = [re.sub(r"\[\d+\]", "", n.strip().split()[-1]) for f in m.group(1).split(";") if f.strip() for n in f.split(",")]
    assert names == [n for n, _ in ofk.Epipolar._fields_] == ["mode", "anchor", "anchor_min", "sigma_max", "beam", "weights"]
    # int, double, int, double, double[3], int under the C ABI's alignment: 8 + 8 + 8 + 8 + 24 + 8
    assert C.sizeof(ofk.Epipolar) == 64
    e = ofk.Epipolar
    assert (e.anchor.offset, e.anchor_min.offset, e.sigma_max.offset, e.beam.offset, e.weights.offset) == (8, 16, 24, 32, 56)


def test_epipolar_kernels_are_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for k in (b"k_epi_solve", b"k_pairs_epi", b"k_stream_epi", b"k_pairs_solve", b"k_stream_fuse", b"k_pairs_joint"):
        assert k in blob, k


def test_settings_from_names(built, ofk):
    e = ofk.epipolar_setting()
    assert (e.mode, e.anchor, e.anchor_min, e.sigma_max, list(e.beam), e.weights) == (1, np.inf, 5, ofk.EPI_SIGMA_MAX, [0.0, 0.0, 1.0], 0)
    e = ofk.epipolar_setting(True, 120.0, 8, 0.01, (0.1, 0.0, 1.0), "robust")
    assert (e.mode, e.anchor, e.anchor_min, e.sigma_max, list(e.beam), e.weights) == (1, 120.0, 8, 0.01, [0.1, 0.0, 1.0], 1)
    assert ofk.epipolar_setting(False).mode == 0 and ofk.epipolar_setting(weights=ofk.EPI_W_ROBUST).weights == 1
    with pytest.raises(ValueError):
        ofk.epipolar_setting(weights="huber")


class Recorder:
    """Stands in for ofk.Context: records what a pipeline applies to it."""
    calls = []

    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        def f(*a, **k):
            Recorder.calls.append((name, a, k))
        return f


def test_pipeline_config_defaults_mean_off(built, pkg, ofk, monkeypatch):
    from of_amd import pipeline
    from of_amd.pipeline import PipelineConfig, FlowPipeline, FlowStream
    for cfg in (PipelineConfig(), PipelineConfig.node(), PipelineConfig.of_module(), PipelineConfig.evaluate_exp(), PipelineConfig.baseline_1080p()):
        assert (cfg.epipolar, cfg.epi_anchor_px, cfg.epi_anchor_min, cfg.epi_sigma_max, cfg.epi_weights) == (False, np.inf, 5, ofk.EPI_SIGMA_MAX, "one")
        assert cfg.epipolar_setting() is None
    on = PipelineConfig(epipolar=True, epi_anchor_px=120.0, epi_anchor_min=8, epi_sigma_max=0.02, epi_weights="robust", range_beam=(0.0, 0.1, 1.0))
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params())         # to_params() does not know the setting
    e = on.epipolar_setting()
    assert (e.mode, e.anchor, e.anchor_min, e.sigma_max, list(e.beam), e.weights) == (1, 120.0, 8, 0.02, [0.0, 0.1, 1.0], 1)
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    for make in (lambda c: FlowPipeline(64, 48, batch=1, cfg=c), lambda c: FlowStream(64, 48, batch=1, cfg=c)):
        Recorder.calls = []
        p = make(PipelineConfig())
        assert not [c for c in Recorder.calls if c[0] == "set_epipolar"]        # the context is left untouched
        assert hasattr(p, "structure")
        make(on)
        sets = [c for c in Recorder.calls if c[0] == "set_epipolar"]
        assert len(sets) == 1 and sets[0][1][0].mode == 1 and sets[0][1][0].anchor == 120.0


def test_optical_fusion_hands_the_epipolar_setting_to_its_pipeline_config(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    from of_amd.velocity_node import optical_fusion, solve_lgs_epipolar
    from of_amd import simulation
    assert optical_fusion(spin=False)._epipolar == {}
    node = optical_fusion(spin=False, epipolar=dict(anchor_px=120.0, sigma_max=0.02, weights="robust"))
    assert node._epipolar == dict(epipolar=True, epi_anchor_px=120.0, epi_sigma_max=0.02, epi_weights="robust") and node.last_epipolar is None
    e = PipelineConfig(**node._epipolar).epipolar_setting()      # every key is one PipelineConfig takes
    assert (e.mode, e.anchor, e.sigma_max, e.weights) == (1, 120.0, 0.02, 1)
    assert optical_fusion(spin=False, epipolar=True)._epipolar == dict(epipolar=True)
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, epipolar=dict(sigma_gyro=1.0))
    assert callable(solve_lgs_epipolar) and callable(simulation.solve_lgs_epipolar)


def values(e):
    return [e.mode, e.anchor, e.anchor_min, e.sigma_max, list(e.beam), e.weights]


@pytest.mark.gpu
def test_setting_round_trip_every_refusal_and_off_after_null(pkg, ofk):
    ctx = ofk.Context(0, 64, 48, 2, 100, 2)
    try:
        assert ctx.get_epipolar().mode == 0                      # off
        with pytest.raises(ofk.OfkError) as e:                   # no run with the setting on yet
            ctx.epipolar_download(1)
        assert e.value.code == ofk.E_INVALID
        good = dict(mode=1, anchor=0.25, anchor_min=2, sigma_max=0.05, beam=(0.0, 0.1, 1.0), weights=1)

        def make(**over):
            d = dict(good, **over)
            return ofk.Epipolar(d["mode"], d["anchor"], d["anchor_min"], d["sigma_max"], (C.c_double * 3)(*d["beam"]), d["weights"])
        ctx.set_epipolar(make())
        assert values(ctx.get_epipolar()) == values(make())
        nan, inf = float("nan"), float("inf")
        x = np.array([[0.5, 0.4], [-0.5, -0.4], [0.5, -0.4], [-0.3, 0.4], [0.01, 0.02]]); u = x * 1e-2 + 1e-3
        kw = dict(d=1.0, nrm=(0.0, 0.0, 1.0), omega=(0.0, 0.0, 0.0))
        for bad in (dict(mode=2), dict(mode=-1), dict(weights=2), dict(weights=-1), dict(anchor=0.0), dict(anchor=-1.0), dict(anchor=nan),
                    dict(anchor_min=0), dict(anchor_min=-3), dict(sigma_max=0.0), dict(sigma_max=-0.1), dict(sigma_max=nan),
                    dict(beam=(0.0, 0.0, 0.0)), dict(beam=(nan, 0.0, 1.0)), dict(beam=(0.0, inf, 1.0))):
            for call in (ctx.set_epipolar, lambda s: ctx.velocity_solve_epipolar(ofk.SOLVE_NODE, x, u, epipolar=s, **kw)):
                with pytest.raises(ofk.OfkError) as e:
                    call(make(**bad))
                assert e.value.code == ofk.E_INVALID, bad
            assert values(ctx.get_epipolar()) == values(make()), bad                  # the previous setting is in place
        with pytest.raises(ofk.OfkError):                        # off is no mode for the stage entry
            ctx.velocity_solve_epipolar(ofk.SOLVE_NODE, x, u, epipolar=make(mode=0), **kw)
        with pytest.raises(ofk.OfkError):                        # OFMODULE is not the sensor model
            ctx.velocity_solve_epipolar(ofk.SOLVE_OFMODULE, x, u, epipolar=make(), **kw)
        out, rec, pts = ctx.velocity_solve_epipolar(ofk.SOLVE_NODE, x, u, epipolar=make(anchor=inf, sigma_max=inf), **kw)
        assert out.shape == (8,) and rec.shape == (32,) and pts.shape == (5, 4)
        assert values(ctx.get_epipolar()) == values(make())      # the stage entry touches no setting
        ctx.set_epipolar(make(anchor=inf, sigma_max=inf, anchor_min=1, beam=(0.0, 0.0, 1e-150)))    # the ends of every range are inside
        ctx.set_epipolar(None)
        assert ctx.get_epipolar().mode == 0 and ctx.get_epipolar().anchor == inf
        ctx.set_epipolar(anchor=50.0)
        assert values(ctx.get_epipolar()) == [1, 50.0, 5, ofk.EPI_SIGMA_MAX, [0.0, 0.0, 1.0], 0]
    finally:
        ctx.close()
