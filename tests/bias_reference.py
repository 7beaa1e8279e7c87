"""tests/bias_reference.py — numpy reference of a stream's gyro bias (ofk.h: ofk_set_gyro_bias; DESIGN.md "gyro bias"): the apply and
the filter step, on top of joint_reference.joint_solve.

Model: omega_true = omega_gyro - b, b a random walk of variance q per step, the gyro's white noise sigma_gyro.  State b^ (3), P (3 x 3).
  apply        omega_used = omega_raw - b^
  filter step  joint_solve at omega_used with the estimated axes free and the held ones held: delta, C_omega.  Predict P_kk += q on the
               estimated axes E; flag 1 / 2 of the solve: nothing more; z = -delta_E, R = C_omega,EE + sigma_gyro^2 I, S = P_EE + R,
               NIS = z^T S^-1 z (gate: flag 3), K = P_.E S^-1, b^ += K z, P_EE := R (S^-1 P)_EE, symmetrised.
The inverse of S comes from numpy's eigh where the device runs a cyclic Jacobi: close, not bit-identical.
Nothing here imports the package: the tests feed it what the device downloaded."""
import numpy as np

import joint_reference as jr

BIAS_DOUBLES = 32


def setting(sigma_flow=2e-4, sigma_gyro=0.0, q=0.0, p0=1e-2, b0=0.0, nis_max=0.0, update=True):
    """The setting as a dict (sigma_flow in the units of the points)."""
    return dict(sigma_flow=float(sigma_flow), sigma_gyro=float(sigma_gyro), q=float(q), p0=np.broadcast_to(np.asarray(p0, np.float64), (3,)).copy(),
                b0=np.broadcast_to(np.asarray(b0, np.float64), (3,)).copy(), nis_max=float(nis_max), update=bool(update))


def initial_state(s):
    st = np.zeros(BIAS_DOUBLES)
    st[0:3] = s["b0"]; st[[3, 6, 8]] = s["p0"] ** 2
    return st


def apply(state, omega_raw):
    """The record behind the apply kernel: raw omega, omega used, flag 4, one more step."""
    r = np.array(state, np.float64)
    raw = np.asarray(omega_raw, np.float64)
    r[9:12] = raw; r[12:15] = raw - r[0:3]; r[15:18] = 0.0; r[18] = 4.0; r[19] = 0.0; r[21] += 1.0; r[22:] = 0.0
    return r


def filter_step(s, r, joint):
    """The filter step on the applied record r with the joint solve's dict (flag, rec).  Returns the record."""
    r = np.array(r, np.float64)
    est = s["p0"] > 0
    if not (s["update"] and est.any()):
        return r
    b = r[0:3].copy(); P = jr.untri(r[3:9])
    P[np.diag_indices(3)] += np.where(est, s["q"], 0.0)
    r[3:9] = jr.tri(P)
    rec = joint["rec"]
    r[28] = rec[11]
    if rec[10] != 0:
        r[18] = rec[10]
        return r
    E = np.flatnonzero(est)
    z = np.zeros(3); z[E] = -rec[3:6][E]
    R = np.zeros((3, 3)); S = np.zeros((3, 3))
    R[np.ix_(E, E)] = jr.untri(rec[15:21])[np.ix_(E, E)] + s["sigma_gyro"] ** 2 * np.eye(len(E))
    S[np.ix_(E, E)] = P[np.ix_(E, E)] + R[np.ix_(E, E)]
    if not np.all(np.isfinite(S)):
        r[18] = 2.0
        return r
    Si, ls = jr._sym_inverse(S, len(E))
    if np.any(~(ls[:len(E)] > 0)):
        r[18] = 2.0
        return r
    nis = float(z @ (Si @ z))
    if not np.isfinite(nis):
        r[18] = 2.0
        return r
    r[19] = nis; r[22:28] = jr.tri(R)
    if s["nis_max"] > 0 and not nis <= s["nis_max"]:
        r[18] = 3.0
        return r
    K = P @ Si
    b = b + K @ z
    Pn = P.copy()                                                # R S^-1 P = P - P S^-1 P as a product: nothing cancels under a wide prior
    Pn[np.ix_(E, E)] = (R @ (Si @ P))[np.ix_(E, E)]
    Pn = 0.5 * (Pn + Pn.T)
    r[0:3] = b; r[3:9] = jr.tri(Pn); r[15:18] = rec[3:6]; r[18] = 0.0; r[20] += 1.0
    return r


def step(s, state, variant, x, u, d, nrm, omega_raw, valid=None, w=None, v_s=None, rss_s=None, rank=None, sigma_flow=None, usable=True):
    """One step: apply, the (plain or given) solve at the corrected omega, the filter step.  w: final robust weights; v_s, rss_s, rank:
    the solve's own outputs (None: joint_reference.plain_solve's).  Returns (record, joint_solve's dict)."""
    r = apply(state, omega_raw)
    sv = np.where(s["p0"] > 0, np.inf, 0.0)
    j = jr.joint_solve(variant, x, u, d, nrm, r[12:15], s["sigma_flow"] if sigma_flow is None else sigma_flow, sv, v_s=v_s, rss_s=rss_s,
                       rank=rank, valid=valid, w=w, usable=usable)
    return filter_step(s, r, j), j


def batch_fusion(s, omega_raw, omega_hat, Rs):
    """With q = 0 the filter over T steps is the information fusion of the prior and the T measurements omega_raw_k - omega^_k with
    covariances R_k, on the estimated axes: (P0^-1 + sum R_k^-1)^-1 (P0^-1 b0 + sum R_k^-1 (omega_raw_k - omega^_k)).  Returns b, P."""
    E = np.flatnonzero(s["p0"] > 0)
    b = s["b0"].copy(); P = np.zeros((3, 3))
    if not len(E):
        return b, P
    J = np.diag(1.0 / s["p0"][E] ** 2); h = J @ s["b0"][E]
    for raw, hat, R in zip(omega_raw, omega_hat, Rs):
        Ri = np.linalg.inv(np.asarray(R)[np.ix_(E, E)])
        J = J + Ri; h = h + Ri @ (np.asarray(raw) - np.asarray(hat))[E]
    PE = np.linalg.inv(J)
    b[E] = PE @ h; P[np.ix_(E, E)] = PE
    return b, P


def rel_dev(b, P, b_ref, P_ref):
    """The deviation TOL_BIAS is stated in: the larger of |b - b_ref| / |b_ref| and |P - P_ref|_F / |P_ref|_F (0 where the reference is 0
    and the value too)."""
    def one(a, ref):
        na, nr = np.linalg.norm(np.asarray(a) - ref), np.linalg.norm(ref)
        return 0.0 if na == 0 else na / nr if nr > 0 else np.inf
    return max(one(b, b_ref), one(P, P_ref))
