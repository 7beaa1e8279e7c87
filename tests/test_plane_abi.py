"""The plane solve's entry points exist in the header, the binding and the library; the setting's structure has the C ABI's size; the
pipeline configuration carries the setting with defaults that mean "off"; optical_fusion hands it down.  On the GPU (a context needs
one): get after set, every refusal rule, a refused setting leaves the previous one in place."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_plane", "ofk_get_plane", "ofk_plane_download", "ofk_velocity_solve_plane")
FIELDS = ["mode", "sigma_flow", "sigma_normal", "sigma_max", "beam", "iters"]


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
    for name, val in (("OFK_PLANE_OFF", 0), ("OFK_PLANE_ON", 1), ("OFK_PLANE_DOUBLES", 32)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
    assert (ofk.PLANE_OFF, ofk.PLANE_ON, ofk.PLANE_DOUBLES) == (0, 1, 32)
    m = re.search(r"typedef struct ofk_plane \{([^}]*)\} ofk_plane;", txt)
    assert m
    names = [re.sub(r"\[\d+\]", "", n.strip().split()[-1]) for f in m.group(1).split(";") if f.strip() for n in f.split(",")]
    # OFK_IMU_STATE carries no variance of the normal, so there is no normal_from_imu field (ofk.h)
    assert names == [n for n, _ in ofk.Plane._fields_] == FIELDS
    # int, 6 doubles (beam[3] among them), int under the C ABI's alignment: 8 + 48 + 8
    assert C.sizeof(ofk.Plane) == 64
    assert [getattr(ofk.Plane, f).offset for f in FIELDS] == [0, 8, 16, 24, 32, 56]
    assert lib.ofk_version() == 100


def test_plane_kernels_are_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for k in (b"k_plane_solve", b"k_pairs_plane", b"k_stream_plane", b"k_pairs_solve", b"k_stream_fuse", b"k_pairs_joint"):
        assert k in blob, k


def values(p):
    return [p.mode, p.sigma_flow, p.sigma_normal, p.sigma_max, list(p.beam), p.iters]


def test_settings_from_names(built, ofk):
    assert values(ofk.plane_setting()) == [1, 0.2, np.inf, 0.1, [0.0, 0.0, 1.0], 6]
    assert values(ofk.plane_setting(True, 0.3, 0.05, sigma_max=np.inf, beam=(0.0, 0.6, 0.8), iters=3)) == [1, 0.3, 0.05, np.inf, [0.0, 0.6, 0.8], 3]
    assert ofk.plane_setting(sigma_normal=0.0).sigma_normal == 0.0
    assert ofk.plane_setting(False).mode == 0


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
        assert (cfg.plane, cfg.plane_sigma_flow_px, cfg.normal_prior, cfg.plane_sigma_max, tuple(cfg.range_beam), cfg.plane_iters) == \
            (False, 0.2, None, 0.1, (0, 0, 1), 6)
        assert cfg.plane_setting() is None
    on = PipelineConfig(plane=True, plane_sigma_flow_px=0.3, normal_prior=0.05, plane_sigma_max=0.2, range_beam=(0.0, 0.6, 0.8), plane_iters=4)
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params())         # to_params() does not know the setting
    assert values(on.plane_setting()) == [1, 0.3, 0.05, 0.2, [0.0, 0.6, 0.8], 4]
    assert PipelineConfig(plane=True).plane_setting().sigma_normal == np.inf
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    for make in (lambda c: FlowPipeline(64, 48, batch=1, cfg=c), lambda c: FlowStream(64, 48, batch=1, cfg=c)):
        Recorder.calls = []
        p = make(PipelineConfig())
        assert not [c for c in Recorder.calls if c[0] == "set_plane"]           # the context is left untouched
        assert hasattr(p, "planes")
        make(on)
        sets = [c for c in Recorder.calls if c[0] == "set_plane"]
        assert len(sets) == 1 and sets[0][1][0].mode == 1 and sets[0][1][0].sigma_flow == 0.3


def test_optical_fusion_hands_the_plane_setting_to_its_pipeline_config(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    from of_amd.velocity_node import optical_fusion, solve_lgs_plane
    from of_amd import simulation
    assert optical_fusion(spin=False)._plane == {}
    node = optical_fusion(spin=False, plane=dict(sigma_flow_px=0.3, normal_prior=0.05, sigma_max=0.2, iters=4))
    assert node._plane == dict(plane=True, plane_sigma_flow_px=0.3, normal_prior=0.05, plane_sigma_max=0.2, plane_iters=4) and node.last_plane is None
    p = PipelineConfig(**node._plane).plane_setting()            # every key is one PipelineConfig takes
    assert values(p) == [1, 0.3, 0.05, 0.2, [0.0, 0.0, 1.0], 4]
    assert optical_fusion(spin=False, plane=True)._plane == dict(plane=True)
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, plane=dict(sigma_tilt=1.0))
    assert callable(solve_lgs_plane) and callable(simulation.solve_lgs_plane)


@pytest.mark.gpu
def test_setting_round_trip_every_refusal_and_off_after_null(pkg, ofk):
    ctx = ofk.Context(0, 64, 48, 2, 100, 2)
    try:
        assert ctx.get_plane().mode == 0                         # off
        with pytest.raises(ofk.OfkError) as e:                   # no run with the setting on yet
            ctx.plane_download(1)
        assert e.value.code == ofk.E_INVALID
        good = dict(mode=1, sigma_flow=0.25, sigma_normal=0.05, sigma_max=0.2, beam=(0.0, 0.6, 0.8), iters=4)

        def make(**over):
            d = dict(good, **over)
            return ofk.Plane(d["mode"], d["sigma_flow"], d["sigma_normal"], d["sigma_max"], (C.c_double * 3)(*d["beam"]), d["iters"])
        ctx.set_plane(make())
        assert values(ctx.get_plane()) == values(make())
        nan, inf = float("nan"), float("inf")
        x = np.array([[0.5, 0.4], [-0.5, -0.4], [0.5, -0.4], [-0.3, 0.4]]); u = np.full((4, 2), 1e-3)
        kw = dict(d=1.0, nrm=(0.0, 0.0, 1.0), omega=(0.0, 0.0, 0.0))
        for bad in (dict(mode=2), dict(mode=-1), dict(sigma_flow=0.0), dict(sigma_flow=-0.1), dict(sigma_flow=nan), dict(sigma_flow=inf),
                    dict(sigma_normal=-0.01), dict(sigma_normal=nan), dict(sigma_normal=-inf), dict(sigma_max=0.0), dict(sigma_max=-0.1),
                    dict(sigma_max=nan), dict(beam=(0.0, 0.0, 0.0)), dict(beam=(0.0, nan, 1.0)), dict(beam=(inf, 0.0, 1.0)), dict(iters=0),
                    dict(iters=17), dict(iters=-1)):
            for call in (ctx.set_plane, lambda p: ctx.velocity_solve_plane(ofk.SOLVE_NODE, x, u, plane=p, **kw)):
                with pytest.raises(ofk.OfkError) as e:
                    call(make(**bad))
                assert e.value.code == ofk.E_INVALID, bad
            assert values(ctx.get_plane()) == values(make()), bad                     # the previous setting is in place
        with pytest.raises(ofk.OfkError):                        # off is no mode for the stage entry
            ctx.velocity_solve_plane(ofk.SOLVE_NODE, x, u, plane=make(mode=0), **kw)
        with pytest.raises(ofk.OfkError):                        # OFMODULE is not the sensor model
            ctx.velocity_solve_plane(ofk.SOLVE_OFMODULE, x, u, plane=make(), **kw)
        out, rec = ctx.velocity_solve_plane(ofk.SOLVE_NODE, x, u, plane=make(), **kw)
        assert out.shape == (8,) and rec.shape == (32,)
        # wgt is there for the solve entries' common signature and must be NULL
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        d1, n1, o1, w1 = np.array([1.0]), np.array([0.0, 0.0, 1.0]), np.zeros(3), np.ones(4)
        o8, r32, pv = np.zeros(8), np.zeros(32), make()
        call = lambda wgt: ctx._L.ofk_velocity_solve_plane(ctx._h, ofk.SOLVE_NODE, vp(x), vp(u), None, 1, 4, vp(d1), vp(n1), vp(o1), None, wgt, None,
                                                           C.byref(pv), vp(o8), vp(r32))
        assert call(vp(w1)) == ofk.E_INVALID and not o8.any()
        assert call(None) == ofk.OK and np.array_equal(o8, out) and np.array_equal(r32, rec)
        assert values(ctx.get_plane()) == values(make())         # the stage entry touches no setting
        ctx.set_plane(make(sigma_normal=inf, sigma_max=inf, sigma_flow=1e-300, iters=16))          # the ends of every range are inside
        ctx.set_plane(make(sigma_normal=0.0, iters=1))
        ctx.set_plane(None)
        assert ctx.get_plane().mode == 0 and ctx.get_plane().iters == 1
        ctx.set_plane(sigma_flow=0.5)
        assert values(ctx.get_plane()) == [1, 0.5, inf, 0.1, [0.0, 0.0, 1.0], 6]
    finally:
        ctx.close()
