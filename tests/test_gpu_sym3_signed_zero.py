"""The symmetric 3 x 3 algebra of csrc/k_lstsq.inc where a reassociated sum could change a zero's sign: tests/sym3_cases.py's
mirror-symmetric point sets, whose normal matrix has exact zeros and whose eigenvector matrix keeps exact zeros beside a negative entry.

CPU (unmarked): the cases are what they claim - m01 == m02 == 0.0, m12 != 0.0, V with an exact zero and a negative entry - and the two
inverses of the restatement differ there in nothing but the sign of zeros.
GPU: records compared with the restatement as uint64 (point_stage_helpers.bits: -0.0 != 0.0), batch 2 per size.  The plain solve,
the residual-mode covariance and the depth step's map solve go through sym3_cases' operation-by-operation restatement of the Jacobi;
the depth step's other slots and its state through tests/track_depth_reference.py, which states them as the device's bits.
Not here: the joint solve (an axis held or none), the plane solve and the keyframe-rotation step on these points.  Their restatements
(joint_reference, plane_reference, keyframe_rot_reference) take their inverses from numpy's eigh and their products from BLAS and are,
by their own words, close to the device and not its bits: on the commit before the helpers were shared all 30 of those records
differed from them in last bits (at most 1.5e-15 of a record's largest entry), none in the sign of a zero, so as uint64 they say nothing
about the helpers.  Those entries are covered by the tolerance tests of their own files."""
import numpy as np
import pytest

import sym3_cases as sc
import track_depth_reference as TD
from point_stage_helpers import bits

gpu = pytest.mark.gpu


def batch2(n):
    cs = [sc.case(n, p) for p in range(2)]
    return np.stack([c[0] for c in cs]), np.stack([c[1] for c in cs])


@pytest.mark.parametrize("n", sc.NS)
def test_cases_have_exact_zeros_and_a_negative_eigenvector_entry(n):
    for problem in range(2):
        x, u = sc.case(n, problem)
        assert np.array_equal(x[0::2] * [-1.0, 1.0], x[1::2]) and np.array_equal(u[0::2] * [-1.0, 1.0], u[1::2])
        m6, g, cnt = sc.sums(x, u)
        assert m6[1] == 0.0 and m6[2] == 0.0 and m6[4] != 0.0, (n, problem, m6)
        v, rank, s3, lam, V = sc.solve(m6, g, cnt)
        V = np.array(V)
        assert rank == 3 and (V == 0.0).any() and (V < 0.0).any(), (n, problem, V)
        A, B = sc.eig_inverse3(lam, V), sc.joint_inverse(lam, V, 3)
        assert np.array_equal(A, B) and (A == 0.0).any()          # equal as numbers: the two orders can differ in a zero's sign alone


@gpu
@pytest.mark.parametrize("n", sc.NS)
def test_plain_solve_and_residual_covariance_bits(gpu_ctx, ofk, n):
    x, u = batch2(n)
    kw = dict(d=[sc.D] * 2, nrm=[sc.NRM] * 2, omega=[sc.OM] * 2)
    out = gpu_ctx.velocity_solve(ofk.SOLVE_NODE, x, u, **kw)
    out_c, cov = gpu_ctx.velocity_solve_cov(ofk.SOLVE_NODE, x, u, mode="residual", **kw)
    assert np.array_equal(bits(out_c), bits(out))
    for b in range(2):
        m6, g, cnt = sc.sums(x[b], u[b])
        v, rank, s3, lam, V = sc.solve(m6, g, cnt)
        want = np.concatenate([v, [out[b, 3], rank], s3])        # the residual is the device's own: it is no part of the 3 x 3 algebra
        assert np.array_equal(bits(out[b]), bits(want)), (n, b, out[b], want)
        want_c = sc.cov_residual_record(m6, cnt, out[b, 3])
        assert np.array_equal(bits(cov[b]), bits(want_c)), (n, b, cov[b], want_c)


@gpu
@pytest.mark.parametrize("n", sc.NS)
def test_track_depth_map_solve_bits(gpu_ctx, ofk, n):
    x, u = batch2(n)
    s = TD.setting(min_rows=3)
    rho0 = 0.4
    state = dict(rho=np.full((2, n), rho0), var=np.full((2, n), (0.1 * rho0) ** 2), nobs=np.full((2, n), 5, np.int32))
    status = np.ones((2, n), np.uint8)
    v_in = np.array([[0.01, 0.3, -0.2], [0.0, 0.29, -0.21]])
    got, rec = gpu_ctx.track_depth_step(x, u, status, [n, n], [sc.OM] * 2, v_in, [1, 1], state, track_depth=ofk.track_depth_setting(
        True, s["sigma_flow"], s["b_min"], s["gate"], s["q"], s["min_obs"], s["rel_max"], s["min_rows"], s["update"]))
    sf2 = float(s["sigma_flow"]) * float(s["sigma_flow"])
    for b in range(2):
        wst, wrec, count, dg = TD.step({k: state[k][b] for k in state}, x[b], u[b], status[b], n, sc.OM, v_in[b], True, s)
        assert dg["mature"].all() and wrec[3] == 0.0
        m6, g, cnt = sc.sums(x[b], u[b], sA=rho0, sB=1.0)
        vm, rank, s3, lam, V = sc.solve(m6, g, cnt)
        wrec[0:3] = vm; wrec[10:16] = sc.tri(sf2 * sc.eig_inverse3(lam, V))
        assert np.array_equal(bits(rec[b]), bits(wrec)), (n, b, rec[b], wrec)
        for k in ("rho", "var", "nobs"):
            assert np.array_equal(bits(got[k][b, :count]), bits(wst[k][:count])), (n, b, k)
