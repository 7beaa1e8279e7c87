"""tests/sym3_cases.py — point sets whose normal matrix has exact zeros, and the kernels' symmetric 3 x 3 algebra restated operation by
operation (csrc/k_lstsq.inc: jacobi3, eig_inverse3, joint_inverse, eig_solve3, rank_cut, solve_from_acc).

The points come in pairs (+x, y), (-x, y) in adjacent rows under the normal (0, 0, 1) and omega = 0, with flows of the same symmetry.
A pair's terms -x y and -x of M cancel exactly, and they still do at the end of the reduction: the butterfly's steps 32 ... 2 add even
lanes to even and odd to odd in the same pattern, so lane 2k holds S and lane 2k + 1 holds -S when the last step adds them.  So m01 and
m02 are exactly 0, m12 is not, the cyclic Jacobi rotates the (1, 2) plane alone, and V keeps exact zeros beside a negative entry:
products V[i][k] V[j][k] / lam[k] that are zeros of either sign, where (t0 + t1) + t2 and ((0.0 + t0) + t1) + t2 differ in the sign
of the result.  Random scenes never get there.

Every function here works on Python floats: IEEE doubles, one rounding per + - * / and sqrt, no contraction - what the device build
(-ffp-contract=off -fno-fast-math) computes.  Nothing here imports the package; the oracle supplies the flow."""
import math

import numpy as np

from joint_reference import EPS, kernel_sum, tri, untri
from oracle import estimation_oracle as eo

NS = (4, 8, 66)                                                  # 66: the last pair lies in the second wave
D, NRM, OM = 1.5, (0.0, 0.0, 1.0), (0.0, 0.0, 0.0)
V_TRUE = (0.0, 0.3, -0.2)                                        # a motion in the mirror plane: its flow has the points' symmetry


def case(n, problem=0):
    """x, u [n, 2]: rows 2k and 2k + 1 are (+x, y) and (-x, y) with flows (ux, uy) and (-ux, uy)."""
    rng = np.random.default_rng(1000 * n + problem)
    h = n // 2
    xs, ys = rng.uniform(0.1, 0.7, h), rng.uniform(-0.5, 0.7, h)
    uh = eo.generate_test_data(np.stack([xs, ys], 1), V_TRUE, OM, D, NRM) + rng.normal(0, 1e-3, (h, 2))     # the +x half; the other mirrors it
    ux, uy = uh[:, 0], uh[:, 1]
    x, u = np.empty((n, 2)), np.empty((n, 2))
    x[0::2, 0], x[1::2, 0], x[0::2, 1], x[1::2, 1] = xs, -xs, ys, ys
    u[0::2, 0], u[1::2, 0], u[0::2, 1], u[1::2, 1] = ux, -ux, uy, uy
    return x, u


def sums(x, u, sA=1.0, sB=D):
    """acc_point's M (6), g (3) and count over all rows at omega = 0 (q = (u, 0)), added in the kernels' order."""
    X, Y = x[:, 0], x[:, 1]
    q0, q1, q2 = u[:, 0], u[:, 1], np.zeros(len(x))
    c0 = Y * q2 - q1; c1 = q0 - X * q2; c2 = X * q1 - Y * q0                     # X q
    t0 = Y * c2 - c1; t1 = c0 - X * c2; t2 = X * c1 - Y * c0                     # X X q
    pp = X * X + Y * Y + 1.0
    sa2 = sA * sA; sab = sA * sB
    terms = np.stack([sa2 * (pp - X * X), sa2 * (-X * Y), sa2 * (-X), sa2 * (pp - Y * Y), sa2 * (-Y), sa2 * (pp - 1.0),
                      -(sab * t0), -(sab * t1), -(sab * t2)], 1)
    s = kernel_sum(terms, np.arange(len(x)))
    return s[:6], s[6:9], float(len(x))


def jacobi3(M):
    """The cyclic Jacobi of k_lstsq.inc: lam descending, V's columns the eigenvectors."""
    A = [[float(M[i][j]) for j in range(3)] for i in range(3)]
    V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(32):
        off = abs(A[0][1]) + abs(A[0][2]) + abs(A[1][2])
        if off <= 1e-20 * (abs(A[0][0]) + abs(A[1][1]) + abs(A[2][2])):
            break
        for p in range(2):
            for q in range(p + 1, 3):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0); s = t * c
                for k in range(3):
                    akp, akq = A[k][p], A[k][q]; A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq
                for k in range(3):
                    apk, aqk = A[p][k], A[q][k]; A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk
                for k in range(3):
                    vkp, vkq = V[k][p], V[k][q]; V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq
    o, d = [0, 1, 2], [A[0][0], A[1][1], A[2][2]]
    for i in range(2):
        for j in range(2 - i):
            if d[o[j]] < d[o[j + 1]]:
                o[j], o[j + 1] = o[j + 1], o[j]
    return [d[o[k]] for k in range(3)], [[V[i][o[k]] for k in range(3)] for i in range(3)]


def eig_inverse3(lam, V):
    return np.array([[(V[i][0] * V[j][0] / lam[0] + V[i][1] * V[j][1] / lam[1]) + V[i][2] * V[j][2] / lam[2] for j in range(3)] for i in range(3)])


def joint_inverse(lam, V, take):
    Ai = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            t = 0.0
            for k in range(take):
                t += V[i][k] * V[j][k] / lam[k]
            Ai[i, j] = t
    return Ai


def eig_solve3(lam, V, g, keep=(True, True, True)):
    x = [0.0, 0.0, 0.0]
    for k in range(3):
        if keep[k]:
            c = (V[0][k] * g[0] + V[1][k] * g[1] + V[2][k] * g[2]) / lam[k]
            for i in range(3):
                x[i] += c * V[i][k]
    return np.array(x)


def solve(m6, g, cnt):
    """solve_from_acc on finite sums: v, rank, s3, and the decomposition."""
    lam, V = jacobi3(untri(m6))
    rows = 3.0 * cnt
    tol = lam[0] * EPS * (rows if rows > 3.0 else 3.0)
    keep = [l > tol and l > 0.0 for l in lam]
    s3 = np.array([math.sqrt(l) if l > 0.0 else 0.0 for l in lam])
    return eig_solve3(lam, V, [float(t) for t in g], keep), sum(keep), s3, lam, V


def cov_residual_record(m6, cnt, rss):
    """The 24-double record of ofk_velocity_solve_cov in residual mode with every sigma 0 and no lever arm: C_v = C_uav = s^2 M^-1.
    Every other term of cov_finish's sums is a zero, and x + (+0.0) keeps x's bits unless x is -0.0, which it turns into +0.0."""
    lam, V = jacobi3(untri(m6))
    s2 = rss / (2.0 * cnt - 3.0)
    Cf = s2 * eig_inverse3(lam, V)
    rec = np.zeros(24)
    rec[0:6] = rec[6:12] = tri(Cf + 0.0); rec[12] = s2
    rec[16] = ((0.0 + Cf[0, 0]) + Cf[1, 1]) + Cf[2, 2]
    return rec
