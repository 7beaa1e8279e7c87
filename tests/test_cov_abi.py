"""CPU-only: the covariance entry points exist in the header, the binding and the library; the setting's structure has the C ABI's
size; the pipeline configuration carries the setting with defaults that mean "off"; the structures callers already fill keep their
size; optical_fusion hands the setting down."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_cov", "ofk_get_cov", "ofk_cov_download", "ofk_velocity_solve_cov")


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
    assert re.search(r"#define\s+OFK_VERSION\s+100\b", txt) and lib.ofk_version() == 100
    for name, val in (("OFK_COV_OFF", 0), ("OFK_COV_PROPAGATE", 1), ("OFK_COV_RESIDUAL", 2), ("OFK_COV_DOUBLES", 24)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
    assert (ofk.COV_OFF, ofk.COV_PROPAGATE, ofk.COV_RESIDUAL, ofk.COV_DOUBLES) == (0, 1, 2, 24)
    assert ofk.COV_MODES == {"off": 0, "propagate": 1, "residual": 2}
    m = re.search(r"typedef struct ofk_cov \{([^}]*)\} ofk_cov;", txt)
    assert m
    names = [re.sub(r"\[\d+\]", "", n.strip().split()[-1]) for f in m.group(1).split(";") if f.strip() for n in f.split(",")]
    assert names == [n for n, _ in ofk.Cov._fields_]
    # int, 8 doubles (sigma_omega[3] among them), 2 ints, 2 doubles under the C ABI's alignment: 8 + 64 + 8 + 16
    assert C.sizeof(ofk.Cov) == 96
    assert ofk.Cov.sigma_flow.offset == 8 and ofk.Cov.sigma_omega.offset == 32 and ofk.Cov.omega_from_imu.offset == 72 and ofk.Cov.r_floor.offset == 80


def test_cov_kernels_are_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for k in (b"k_cov_solve", b"k_pairs_cov", b"k_stream_cov", b"k_kf_records_cov", b"k_pairs_solve", b"k_stream_fuse"):
        assert k in blob, k


def test_settings_from_names(built, ofk):
    c = ofk.cov_setting()
    assert (c.mode, c.sigma_flow, c.sigma_pos, c.sigma_d, list(c.sigma_omega), c.sigma_normal, c.sigma_offset, c.omega_from_imu, c.filter_r,
            c.r_floor, c.nis_max) == (1, 0.0, 0.0, 0.0, [0.0, 0.0, 0.0], 0.0, 0.0, 0, 0, 0.0, 0.0)
    c = ofk.cov_setting("residual", sigma_d=0.05, sigma_omega=0.01, omega_from_imu=True, filter_r=True, r_floor=1e-6, nis_max=11.3)
    assert (c.mode, c.sigma_d, list(c.sigma_omega), c.omega_from_imu, c.filter_r, c.r_floor, c.nis_max) == (2, 0.05, [0.01] * 3, 1, 1, 1e-6, 11.3)
    assert list(ofk.cov_setting(ofk.COV_PROPAGATE, sigma_omega=(1, 2, 3)).sigma_omega) == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError):
        ofk.cov_setting("bootstrap")
    C6 = ofk.cov_matrix(np.arange(12.0).reshape(2, 6))
    assert C6.shape == (2, 3, 3) and np.array_equal(C6[0], [[0, 1, 2], [1, 3, 4], [2, 4, 5]]) and np.array_equal(C6[1], C6[1].T)


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
    plain = ofk.Params(500, 0.01, 10.0, 7, 15, 3, 20, 0.03, 1e-4, ofk.SOLVE_NODE, 0, 0.0)
    for cfg in (PipelineConfig(), PipelineConfig.node(), PipelineConfig.of_module(), PipelineConfig.evaluate_exp(), PipelineConfig.baseline_1080p()):
        assert (cfg.cov, cfg.sigma_flow_px, cfg.sigma_pos_px, cfg.sigma_d, cfg.sigma_omega, cfg.sigma_normal, cfg.sigma_offset, cfg.omega_from_imu,
                cfg.cov_filter, cfg.r_floor, cfg.nis_max) == ("off", 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, False, False, 0.0, 0.0)
        assert cfg.cov_setting() is None
    on = PipelineConfig(cov="residual", sigma_flow_px=0.3, sigma_pos_px=0.5, sigma_d=0.05, sigma_omega=(0.01, 0.02, 0.03), sigma_normal=0.004,
                        sigma_offset=0.006, omega_from_imu=True, cov_filter=True, r_floor=1e-6, nis_max=16.0)
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params()) == bytes(plain)       # to_params() does not know the setting
    c = on.cov_setting()
    assert (c.mode, c.sigma_flow, c.sigma_pos, c.sigma_d, list(c.sigma_omega), c.sigma_normal, c.sigma_offset, c.omega_from_imu, c.filter_r,
            c.r_floor, c.nis_max) == (2, 0.3, 0.5, 0.05, [0.01, 0.02, 0.03], 0.004, 0.006, 1, 1, 1e-6, 16.0)
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    for make in (lambda c: FlowPipeline(64, 48, batch=1, cfg=c), lambda c: FlowStream(64, 48, batch=1, cfg=c)):
        Recorder.calls = []
        p = make(PipelineConfig())
        assert not [c for c in Recorder.calls if c[0] == "set_cov"]             # the context is left untouched
        assert hasattr(p, "covariances")
        make(on)
        sets = [c for c in Recorder.calls if c[0] == "set_cov"]
        assert len(sets) == 1 and sets[0][1][0].mode == 2 and sets[0][1][0].filter_r == 1


def test_caller_structures_keep_their_size(built, ofk):
    assert C.sizeof(ofk.Params) == 72 and C.sizeof(ofk.Fusion) == 56 and C.sizeof(ofk.Robust) == 40
    txt = open(os.path.join(ROOT, "include", "ofk.h")).read()
    for name, fields in (("ofk_params", ofk.Params._fields_), ("ofk_fusion", ofk.Fusion._fields_)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S)
        assert m, name
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        names = [re.split(r"[\s\*]+", f.strip())[-1] for f in body.split(";") if f.strip()]
        assert names == [n for n, _ in fields], (name, names)


def test_optical_fusion_hands_the_cov_setting_to_its_pipeline_config(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    from of_amd.velocity_node import optical_fusion, solve_lgs_cov
    from of_amd import simulation
    assert optical_fusion(spin=False)._cov == {}
    node = optical_fusion(spin=False, cov=dict(mode="residual", sigma_d=0.05, sigma_omega=0.01, cov_filter=True))
    assert node._cov == dict(cov="residual", sigma_d=0.05, sigma_omega=0.01, cov_filter=True) and node.last_cov is None
    c = PipelineConfig(**node._cov).cov_setting()               # every key is one PipelineConfig takes
    assert (c.mode, c.sigma_d, list(c.sigma_omega), c.filter_r) == (2, 0.05, [0.01] * 3, 1)
    assert optical_fusion(spin=False, cov=dict(sigma_flow_px=0.3))._cov == dict(cov="propagate", sigma_flow_px=0.3)
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, cov=dict(mode="bootstrap"))
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, cov=dict(sigma_speed=1.0))
    assert callable(solve_lgs_cov) and callable(simulation.predict_sweep)
