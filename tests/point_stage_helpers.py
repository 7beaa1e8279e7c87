"""What the GPU tests of the three point corrections (camera model, rolling shutter, finite motion) share: bit patterns, the point
comparison, and the checks of a pair run against the stage entries.  No test file: each scene stays with its tests."""
import numpy as np

import robust_reference as rr
from oracle import estimation_oracle as eo

SENTINEL = np.float32(-7.5)
ROBUST = dict(loss="tukey", c=4.685, iters=5, hypotheses=64, seed=0x1234ABCD5678)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def same_points(got, ref, ulp=0):
    """Finite results within `ulp` float32 steps (0: the same bits); infinities equal; not-a-number where the reference is."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    fin = np.isfinite(ref)
    if not np.array_equal(np.isnan(got), np.isnan(ref)) or not np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)]):
        return False
    if ulp == 0:
        return np.array_equal(bits(got[fin]), bits(ref[fin]))
    return bool(np.all(np.abs(got[fin].astype(np.float64) - ref[fin].astype(np.float64)) <= ulp * np.spacing(np.maximum(np.abs(got[fin]), np.abs(ref[fin])))))


def assert_image_side_identical(a, b, tag):
    assert np.array_equal(a["counts"], b["counts"]), tag
    for k in ("prev_pts", "next_pts", "status", "err"):
        assert np.array_equal(bits(a[k]), bits(b[k])), (tag, k)


def assert_plain_records(out, pu, nu, sensors, tag):
    """The records are the node solve of the points the solve stage saw (pu, nu) with the downloaded status, within 1e-10."""
    for b in range(len(out["counts"])):
        n = int(out["counts"][b]); sr = sensors[b]
        ok = out["status"][b, :n] == 1
        new = nu[b, :n].astype(np.float64); old = pu[b, :n].astype(np.float64)
        x = (new[ok] - [sr[20], sr[21]]) * sr[19]; u = (new[ok] - old[ok]) * sr[19]
        v, _, rank, s = eo.solve_lgs_node(x, u, sr[0], sr[1:4], sr[4:7])
        rec = out["records"][b]
        assert rec[4] == rank and rec[11] == ok.sum() and rec[12] == n and rec[13] == ok.sum(), (tag, b, rec)
        np.testing.assert_allclose(rec[0:3], v, rtol=0, atol=1e-10, err_msg=str((tag, b)))
        np.testing.assert_allclose(rec[8:11], eo.post_solve(v, sr[7:16].reshape(3, 3), sr[4:7], sr[16:19]), rtol=0, atol=1e-10, err_msg=str((tag, b)))
        np.testing.assert_allclose(rec[5:8], s, rtol=1e-9, err_msg=str((tag, b)))


def robust_reference(b, x, u, ok, sr, st):
    """robust_reference's solve of pair b, with the allowance of tests/test_gpu_robust_pipeline.py: two hypotheses whose scores tie to
    1e-12 may be ranked either way, and the reference then follows the device's choice."""
    kw = dict(valid=ok, loss=rr.TUKEY, c=ROBUST["c"], iters=ROBUST["iters"], hypotheses=ROBUST["hypotheses"], seed=ROBUST["seed"], problem=b)
    ref = rr.robust_solve(rr.NODE, x, u, sr[0], sr[1:4], sr[4:7], **kw)
    if int(st[4]) != int(ref["stats"][4]):
        best = ref["stats"][5]
        assert int(st[4]) >= 0 and abs(st[5] - best) <= 1e-12 * best, ("hyp", b, st, ref["stats"])
        ref = rr.robust_solve(rr.NODE, x, u, sr[0], sr[1:4], sr[4:7], force_hyp=int(st[4]), **kw)
    return ref
