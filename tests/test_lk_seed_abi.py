"""CPU-only: the seeded-LK entry points exist in the header, the binding and the library; the cv2 facade takes OpenCV's two LK flags
as far as the point where it needs a device context, and rejects what OpenCV rejects; the pipeline configuration carries the
seed setting with defaults that mean "off"."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_lk_pyr_ex", "ofk_predict_points", "ofk_set_lk_seed", "ofk_get_lk_seed")


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
    for name, val in (("OFK_LK_USE_INITIAL_FLOW", 4), ("OFK_LK_GET_MIN_EIGENVALS", 8), ("OFK_SEED_OFF", 0), ("OFK_SEED_MODEL", 1),
                      ("OFK_SEED_ROTATION", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
    assert (ofk.LK_USE_INITIAL_FLOW, ofk.LK_GET_MIN_EIGENVALS) == (4, 8)
    assert (ofk.SEED_OFF, ofk.SEED_MODEL, ofk.SEED_ROTATION) == (0, 1, 2)


def test_flagged_kernels_are_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for k in (b"k_lk15q_f", b"k_lk15_f", b"k_lk_f", b"k_seed_points", b"k_lk15q", b"k_lk15"):
        assert k in blob, k


class NeedsContext(Exception):
    pass


def test_cv2_facade_takes_the_lk_flags(built, pkg, ofk, monkeypatch):
    import of_amd.cv2_hip as cv2
    assert cv2.OPTFLOW_USE_INITIAL_FLOW == 4 and cv2.OPTFLOW_LK_GET_MIN_EIGENVALS == 8

    def no_context(*a, **k):
        raise NeedsContext()

    monkeypatch.setattr(ofk, "default_context", no_context)
    img = np.zeros((64, 80), np.uint8)
    pts = np.array([[[20.0, 20.0]], [[40.0, 30.0]]], np.float32)
    for flags, nxt in ((0, None), (cv2.OPTFLOW_LK_GET_MIN_EIGENVALS, None), (cv2.OPTFLOW_USE_INITIAL_FLOW, pts + 1),
                       (cv2.OPTFLOW_USE_INITIAL_FLOW | cv2.OPTFLOW_LK_GET_MIN_EIGENVALS, pts + 1)):
        with pytest.raises(NeedsContext):                      # every argument check passed
            cv2.calcOpticalFlowPyrLK(img, img, pts, nxt, winSize=(15, 15), maxLevel=2, flags=flags)
    with pytest.raises(ValueError):                            # unknown bits
        cv2.calcOpticalFlowPyrLK(img, img, pts, None, winSize=(15, 15), flags=1)
    with pytest.raises(ValueError):
        cv2.calcOpticalFlowPyrLK(img, img, pts, pts, winSize=(15, 15), flags=4 | 16)
    with pytest.raises(ValueError):                            # initial flow without nextPts
        cv2.calcOpticalFlowPyrLK(img, img, pts, None, winSize=(15, 15), flags=cv2.OPTFLOW_USE_INITIAL_FLOW)
    with pytest.raises(ValueError):                            # nextPts of another length
        cv2.calcOpticalFlowPyrLK(img, img, pts, pts[:1], winSize=(15, 15), flags=cv2.OPTFLOW_USE_INITIAL_FLOW)
    bad = pts.copy(); bad[0, 0, 0] = np.nan
    with pytest.raises(ValueError):
        cv2.calcOpticalFlowPyrLK(img, img, pts, bad, winSize=(15, 15), flags=cv2.OPTFLOW_USE_INITIAL_FLOW)
    with pytest.raises(NotImplementedError):                   # non-square windows stay unsupported
        cv2.calcOpticalFlowPyrLK(img, img, pts, pts, winSize=(15, 21), flags=cv2.OPTFLOW_USE_INITIAL_FLOW)


def test_pipeline_config_defaults_mean_off(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    for cfg in (PipelineConfig(), PipelineConfig.node(), PipelineConfig.of_module(), PipelineConfig.evaluate_exp(), PipelineConfig.baseline_1080p()):
        assert cfg.lk_seed == "off" and cfg.seed_gain == 1.0
    assert ofk.SEED_MODES == {"off": 0, "model": 1, "rotation": 2}
    with pytest.raises(ValueError):
        ofk._seed_mode("sideways")
