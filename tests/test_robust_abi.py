"""CPU-only: the robust-solve entry points exist in the header, the binding and the library; ofk_robust_pairs draws the reference's
sample; the pipeline configuration carries the setting with defaults that mean "off"; the structures callers already fill keep
their size."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import robust_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_robust", "ofk_get_robust", "ofk_robust_download", "ofk_velocity_solve_robust", "ofk_robust_pairs")


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
    for name, val in (("OFK_ROBUST_OFF", 0), ("OFK_ROBUST_HUBER", 1), ("OFK_ROBUST_TUKEY", 2), ("OFK_ROBUST_MIN_POINTS", 8), ("OFK_ROBUST_DOUBLES", 8)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
    assert (ofk.ROBUST_OFF, ofk.ROBUST_HUBER, ofk.ROBUST_TUKEY, ofk.ROBUST_MIN_POINTS, ofk.ROBUST_DOUBLES) == (0, 1, 2, 8, 8)
    assert ofk.ROBUST_LOSSES == {"off": 0, "huber": 1, "tukey": 2}
    m = re.search(r"typedef struct ofk_robust \{([^}]*)\} ofk_robust;", txt)
    assert m and [f.split()[-1] for f in m.group(1).split(";") if f.strip()] == [n for n, _ in ofk.Robust._fields_]
    assert C.sizeof(ofk.Robust) == 40                            # int, double, int, int, u64, int under the C ABI's alignment


def test_robust_kernels_are_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for k in (b"k_solve_robust", b"k_pairs_robust", b"k_pairs_solve_wg", b"k_pairs_solve", b"k_stream_fuse"):
        assert k in blob, k


@pytest.mark.parametrize("seed,problem,K,m", [(0, 0, 64, 500), (0x1234ABCD5678, 3, 256, 8), (2 ** 64 - 1, 1023, 16, 2), (7, 135, 1, 4096),
                                              (0xDEADBEEF00000001, 2 ** 31, 100, 9), (5, 0, 0, 300)])
def test_robust_pairs_is_the_reference_sample(built, ofk, seed, problem, K, m):
    i, j = ofk.robust_pairs(seed, problem, K, m)
    ri, rj = rr.sample(seed, problem, K, m)
    assert len(i) == K and np.array_equal(i, ri) and np.array_equal(j, rj)
    assert np.all(i != j) and np.all((i >= 0) & (i < m)) and np.all((j >= 0) & (j < m))


def test_robust_pairs_covers_every_pair_and_refuses_bad_arguments(built, ofk):
    seen = set()
    for problem in range(40):
        i, j = ofk.robust_pairs(11, problem, 256, 5)
        seen |= set(zip(i.tolist(), j.tolist()))
    assert seen == {(a, b) for a in range(5) for b in range(5) if a != b}    # j is uniform over the other points, both orders occur
    for K, m in ((4, 1), (4, 0), (4, -3), (-1, 10), (257, 10)):
        with pytest.raises(ofk.OfkError):
            ofk.robust_pairs(0, 0, K, m)
    lib = ofk.load_library()
    assert lib.ofk_robust_pairs(C.c_ulonglong(0), C.c_uint(0), 4, 10, None, None) == -1


def test_settings_from_names(built, ofk):
    r = ofk.robust_setting("tukey")
    assert (r.loss, r.c, r.iters, r.hypotheses, r.seed, r.drop) == (2, 4.685, 5, 64, 0, 0)
    r = ofk.robust_setting("huber", iters=3, hypotheses=0, seed=2 ** 63 + 5, drop=True)
    assert (r.loss, r.c, r.iters, r.hypotheses, r.seed, r.drop) == (1, 1.345, 3, 0, 2 ** 63 + 5, 1)
    assert ofk.robust_setting(ofk.ROBUST_TUKEY, c=3.0).c == 3.0
    with pytest.raises(ValueError):
        ofk.robust_setting("cauchy")


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
        assert (cfg.robust, cfg.robust_c, cfg.robust_iters, cfg.robust_hypotheses, cfg.robust_seed, cfg.robust_drop) == ("off", None, 5, 64, 0, False)
        assert cfg.robust_setting() is None
    on = PipelineConfig(robust="tukey", robust_hypotheses=16, robust_seed=9, robust_drop=True)
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params()) == bytes(plain)       # to_params() does not know the setting
    r = on.robust_setting()
    assert (r.loss, r.c, r.iters, r.hypotheses, r.seed, r.drop) == (2, 4.685, 5, 16, 9, 1)
    assert PipelineConfig(robust="huber").robust_setting().c == 1.345 and PipelineConfig(robust="huber", robust_c=2.0).robust_setting().c == 2.0
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    for make in (lambda c: FlowPipeline(64, 48, batch=1, cfg=c), lambda c: FlowStream(64, 48, batch=1, cfg=c)):
        Recorder.calls = []
        make(PipelineConfig())
        assert not [c for c in Recorder.calls if c[0] == "set_robust"]           # the context is left untouched
        make(on)
        sets = [c for c in Recorder.calls if c[0] == "set_robust"]
        assert len(sets) == 1 and sets[0][1][0].loss == 2 and sets[0][1][0].drop == 1


def test_caller_structures_keep_their_size(built, ofk):
    assert C.sizeof(ofk.Params) == 72 and C.sizeof(ofk.Fusion) == 56       # what they were before the setting existed
    txt = open(os.path.join(ROOT, "include", "ofk.h")).read()
    for name, fields in (("ofk_params", ofk.Params._fields_), ("ofk_fusion", ofk.Fusion._fields_)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S)
        assert m, name
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        names = [re.split(r"[\s\*]+", f.strip())[-1] for f in body.split(";") if f.strip()]
        assert names == [n for n, _ in fields], (name, names)


def test_optical_fusion_hands_the_robust_setting_to_its_pipeline_config(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    from of_amd.velocity_node import optical_fusion
    assert optical_fusion(spin=False)._robust == {}
    node = optical_fusion(spin=False, robust=dict(loss="huber", hypotheses=32, seed=3, drop=True))
    assert node._robust == dict(robust="huber", robust_hypotheses=32, robust_seed=3, robust_drop=True)
    r = PipelineConfig(**node._robust).robust_setting()         # every key is one PipelineConfig takes
    assert (r.loss, r.c, r.iters, r.hypotheses, r.seed, r.drop) == (1, 1.345, 5, 32, 3, 1)
    assert optical_fusion(spin=False, robust=dict(iters=2))._robust == dict(robust="tukey", robust_iters=2)
