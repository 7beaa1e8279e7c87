"""The joint solve's setting of the resident tests and the check of a device record against joint_reference.joint_solve, shared by
tests/test_gpu_joint.py and the tests that run the joint solve behind another setting.  No test file."""
import numpy as np

import joint_reference as jr
from test_joint_reference import TOL

RSS_TOL = 1e-10
REC_TOL = 1e-9
COND_MAX = 1e4
SEEN = dict(dev=0.0)
JOINT = dict(sigma_flow=0.2, sigma_omega=1e-3)


def assert_joint_close(v, rss, rec, ref, tag):
    """The device's v, residual and joint record against joint_solve's dict."""
    assert rec[10] == ref["flag"], (tag, "flag", rec[10], ref["flag"])
    assert rec[11] == ref["rec"][11] and np.all(rec[27:] == 0), tag
    assert np.array_equal(rec[6:10], ref["rec"][6:10]), (tag, "the solve's v and residual before")
    if ref["flag"] != 0:
        assert np.array_equal(rec[0:3], ref["rec"][0:3]) and np.all(rec[3:6] == 0) and np.all(rec[15:27] == 0), tag
        assert np.array_equal(v, ref["v"]) and rss == ref["rss"], (tag, "the record is untouched")
        return
    dev = jr.rel_dev(v, rec[0:3], ref["v"], ref["omega"])
    SEEN["dev"] = max(SEEN["dev"], dev)
    assert dev <= TOL, (tag, dev)
    floor = 3 * rec[11] * ((TOL + 8 * jr.EPS) * ref["scale"]) ** 2
    assert abs(rss - ref["rss"]) <= RSS_TOL * ref["rss"] + floor, (tag, "rss", rss, ref["rss"], floor)
    np.testing.assert_allclose(rec[3:6], ref["rec"][3:6], rtol=0, atol=TOL * np.linalg.norm(ref["omega"]), err_msg=tag)
    for sl in (slice(12, 15), slice(15, 21), slice(21, 27)):
        scale = np.abs(ref["rec"][sl]).max()
        assert np.abs(rec[sl] - ref["rec"][sl]).max() <= REC_TOL * scale, (tag, sl, rec[sl], ref["rec"][sl])
    assert ref["rec"][12] / ref["rec"][12:15][ref["rec"][12:15] > 0].min() < COND_MAX, tag
