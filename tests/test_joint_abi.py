"""The joint velocity and rotation solve's entry points exist in the header, the binding and the library; the setting's structure has
the C ABI's size; the pipeline configuration carries the setting with defaults that mean "off"; optical_fusion hands it down.  On the
GPU (a context needs one): get after set, every refusal rule, a refused setting leaves the previous one in place."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_joint", "ofk_get_joint", "ofk_joint_download", "ofk_velocity_solve_joint")


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
    for name, val in (("OFK_JOINT_OFF", 0), ("OFK_JOINT_ON", 1), ("OFK_JOINT_DOUBLES", 32)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
    assert (ofk.JOINT_OFF, ofk.JOINT_ON, ofk.JOINT_DOUBLES) == (0, 1, 32)
    m = re.search(r"typedef struct ofk_joint \{([^}]*)\} ofk_joint;", txt)
    assert m
    names = [re.sub(r"\[\d+\]", "", n.strip().split()[-1]) for f in m.group(1).split(";") if f.strip() for n in f.split(",")]
    assert names == [n for n, _ in ofk.Joint._fields_] == ["mode", "sigma_flow", "sigma_omega", "omega_from_imu"]
    # int, 4 doubles (sigma_omega[3] among them), int under the C ABI's alignment: 8 + 32 + 8
    assert C.sizeof(ofk.Joint) == 48
    assert ofk.Joint.sigma_flow.offset == 8 and ofk.Joint.sigma_omega.offset == 16 and ofk.Joint.omega_from_imu.offset == 40


def test_joint_kernels_are_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for k in (b"k_joint_solve", b"k_pairs_joint", b"k_stream_joint", b"k_pairs_solve", b"k_stream_fuse", b"k_pairs_cov"):
        assert k in blob, k


def test_settings_from_names(built, ofk):
    j = ofk.joint_setting()
    assert (j.mode, j.sigma_flow, list(j.sigma_omega), j.omega_from_imu) == (1, 0.2, [np.inf] * 3, 0)
    j = ofk.joint_setting(True, 0.3, 1e-3, omega_from_imu=True)
    assert (j.mode, j.sigma_flow, list(j.sigma_omega), j.omega_from_imu) == (1, 0.3, [1e-3] * 3, 1)
    assert list(ofk.joint_setting(sigma_omega=(0.0, 1e-3, np.inf)).sigma_omega) == [0.0, 1e-3, np.inf]
    assert ofk.joint_setting(False).mode == 0


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
        assert (cfg.joint, cfg.joint_sigma_flow_px, cfg.omega_prior, cfg.omega_prior_from_imu) == (False, 0.2, None, False)
        assert cfg.joint_setting() is None
    on = PipelineConfig(joint=True, joint_sigma_flow_px=0.3, omega_prior=(1e-3, 0.0, np.inf), omega_prior_from_imu=True)
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params())         # to_params() does not know the setting
    j = on.joint_setting()
    assert (j.mode, j.sigma_flow, list(j.sigma_omega), j.omega_from_imu) == (1, 0.3, [1e-3, 0.0, np.inf], 1)
    assert list(PipelineConfig(joint=True, omega_prior=2e-3).joint_setting().sigma_omega) == [2e-3] * 3
    assert list(PipelineConfig(joint=True).joint_setting().sigma_omega) == [np.inf] * 3
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    for make in (lambda c: FlowPipeline(64, 48, batch=1, cfg=c), lambda c: FlowStream(64, 48, batch=1, cfg=c)):
        Recorder.calls = []
        p = make(PipelineConfig())
        assert not [c for c in Recorder.calls if c[0] == "set_joint"]           # the context is left untouched
        assert hasattr(p, "rotations")
        make(on)
        sets = [c for c in Recorder.calls if c[0] == "set_joint"]
        assert len(sets) == 1 and sets[0][1][0].mode == 1 and sets[0][1][0].sigma_flow == 0.3


def test_optical_fusion_hands_the_joint_setting_to_its_pipeline_config(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    from of_amd.velocity_node import optical_fusion, solve_lgs_joint
    from of_amd import simulation
    assert optical_fusion(spin=False)._joint == {}
    node = optical_fusion(spin=False, joint=dict(sigma_flow_px=0.3, omega_prior=1e-3))
    assert node._joint == dict(joint=True, joint_sigma_flow_px=0.3, omega_prior=1e-3) and node.last_joint is None
    j = PipelineConfig(**node._joint).joint_setting()            # every key is one PipelineConfig takes
    assert (j.mode, j.sigma_flow, list(j.sigma_omega)) == (1, 0.3, [1e-3] * 3)
    assert optical_fusion(spin=False, joint=True)._joint == dict(joint=True)
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, joint=dict(sigma_gyro=1.0))
    assert callable(solve_lgs_joint) and callable(simulation.solve_lgs_joint)


def values(j):
    return [j.mode, j.sigma_flow, list(j.sigma_omega), j.omega_from_imu]


@pytest.mark.gpu
def test_setting_round_trip_every_refusal_and_off_after_null(pkg, ofk):
    ctx = ofk.Context(0, 64, 48, 2, 100, 2)
    try:
        assert ctx.get_joint().mode == 0                         # off
        with pytest.raises(ofk.OfkError) as e:                   # no run with the setting on yet
            ctx.joint_download(1)
        assert e.value.code == ofk.E_INVALID
        good = dict(mode=1, sigma_flow=0.25, sigma_omega=(1e-3, 0.0, np.inf), omega_from_imu=1)

        def make(**over):
            d = dict(good, **over)
            return ofk.Joint(d["mode"], d["sigma_flow"], (C.c_double * 3)(*d["sigma_omega"]), d["omega_from_imu"])
        ctx.set_joint(make())
        assert values(ctx.get_joint()) == values(make())
        nan, inf = float("nan"), float("inf")
        x = np.array([[0.5, 0.4], [-0.5, -0.4], [0.5, -0.4], [-0.3, 0.4]]); u = np.full((4, 2), 1e-3)
        kw = dict(d=1.0, nrm=(0.0, 0.0, 1.0), omega=(0.0, 0.0, 0.0))
        for bad in (dict(mode=2), dict(mode=-1), dict(sigma_flow=0.0), dict(sigma_flow=-0.1), dict(sigma_flow=nan), dict(sigma_flow=inf),
                    dict(sigma_omega=(-1e-3, 0.0, 0.0)), dict(sigma_omega=(0.0, nan, 0.0)), dict(sigma_omega=(0.0, 0.0, -inf)), dict(omega_from_imu=2)):
            for call in (ctx.set_joint, lambda j: ctx.velocity_solve_joint(ofk.SOLVE_NODE, x, u, joint=j, **kw)):
                with pytest.raises(ofk.OfkError) as e:
                    call(make(**bad))
                assert e.value.code == ofk.E_INVALID, bad
            assert values(ctx.get_joint()) == values(make()), bad                     # the previous setting is in place
        with pytest.raises(ofk.OfkError):                        # off is no mode for the stage entry
            ctx.velocity_solve_joint(ofk.SOLVE_NODE, x, u, joint=make(mode=0), **kw)
        with pytest.raises(ofk.OfkError):                        # OFMODULE is not the sensor model
            ctx.velocity_solve_joint(ofk.SOLVE_OFMODULE, x, u, joint=make(), **kw)
        out, rec = ctx.velocity_solve_joint(ofk.SOLVE_NODE, x, u, joint=make(), **kw)
        assert out.shape == (8,) and rec.shape == (32,)
        assert values(ctx.get_joint()) == values(make())         # the stage entry touches no setting
        ctx.set_joint(make(sigma_omega=(inf, inf, inf), sigma_flow=1e-300))           # the ends of every range are inside
        ctx.set_joint(None)
        assert ctx.get_joint().mode == 0 and ctx.get_joint().sigma_flow == 1e-300
        ctx.set_joint(sigma_flow=0.5)
        assert values(ctx.get_joint()) == [1, 0.5, [inf] * 3, 0]
    finally:
        ctx.close()
