"""The plane solve's setting of the resident tests and the check of a device record against plane_reference.plane_solve, shared by
tests/test_gpu_plane.py and the tests that run the plane solve behind another setting.  No test file."""
import numpy as np

import plane_reference as pr
from test_plane_reference import TOL, COND_MAX

RSS_TOL = 1e-10
REC_TOL = 1e-9
SEEN = dict(dev=0.0)
PLANE = dict(sigma_flow=0.2, sigma_normal=0.2)


def assert_plane_close(v, rss, rec, ref, tag):
    """The device's v, residual and plane record against plane_solve's dict."""
    rr = ref["rec"]
    assert rec[10] == ref["flag"], (tag, "flag", rec[10], ref["flag"], rec[12:15], rr[12:15])
    assert rec[11] == rr[11] and np.all(rec[28:] == 0), tag
    assert np.array_equal(rec[6:10], rr[6:10]), (tag, "the solve's v and residual before")
    if ref["flag"] != 0:
        assert np.array_equal(rec[0:4], rr[0:4]) and np.all(rec[4:6] == 0) and np.all(rec[14:26] == 0), tag
        assert np.array_equal(v, ref["v"]) and rss == ref["rss"], (tag, "the record is untouched")
        return
    dev = pr.rel_dev(v, pr.record_m(rec), ref["v"], ref["m"])
    SEEN["dev"] = max(SEEN["dev"], dev)
    assert dev <= TOL, (tag, dev)
    floor = 3 * rec[11] * ((TOL + 8 * pr.EPS) * ref["scale"]) ** 2
    assert abs(rss - ref["rss"]) <= RSS_TOL * ref["rss"] + floor, (tag, "rss", rss, ref["rss"], floor)
    for k in (26, 27):
        assert abs(rec[k] - rr[k]) <= RSS_TOL * rr[k] + floor, (tag, k, rec[k], rr[k], floor)
    np.testing.assert_allclose(rec[4:6], rr[4:6], rtol=0, atol=TOL * np.linalg.norm(ref["m"]), err_msg=tag)
    for sl in (slice(12, 14), slice(14, 15), slice(15, 16), slice(17, 20), slice(20, 26)):
        scale = np.abs(rr[sl]).max()
        assert np.abs(rec[sl] - rr[sl]).max() <= REC_TOL * scale, (tag, sl, rec[sl], rr[sl])
    assert abs(rec[16] - rr[16]) <= 1e-6 * rr[16] + 1e-11, (tag, "last step", rec[16], rr[16])
    assert ref["cond"] < COND_MAX, (tag, ref["cond"])
