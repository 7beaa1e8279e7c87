"""tests/joint_reference.py — numpy reference of the joint velocity and rotation solve (ofk.h: ofk_set_joint; DESIGN.md "joint solve").

With p = (x, y, 1), X = [p]x, N = X^T X = |p|^2 I - p p^T, q0 = (u, 0) + p x omega0 and the solve's scalings a = sA, b = sB (NODE:
a = 1, b = d / (n.p); SIM: a = n.p, b = d) point i's rows for omega = omega0 + delta are  a X v + b N delta = b X q0.  With the prior
delta_k ~ N(0, sigma_k^2) weighted by the row noise d sigma_f the normal equations are [M, K; K^T, D + Lambda] (v, delta) = (g_v, g_d).

Two routes:
  joint_solve    the arithmetic of ofk.h restated: the 19 sums in the kernel's order (four virtual waves of 64 lanes, the shuffle
                 butterfly, (s0 + s1) + (s2 + s3)), the Schur complement on v_s = the plain solve, the flags, the joint record.  The
                 two 3 x 3 inverses come from numpy's eigh, not from a cyclic Jacobi: close, not bit-identical, to the device.
  joint_lstsq    independent: np.linalg.lstsq on the stacked 3 m + 3 rows (held axes' columns left out, free axes' prior rows zero).
Nothing here imports the package: the tests feed it what the device downloaded."""
import numpy as np

NODE, SIM = 0, 1
JOINT_DOUBLES = 32
EPS = 2.220446049250313e-16


def skew(a):
    a = np.asarray(a, np.float64)
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def point_terms(variant, x, u, d, n, omega):
    x = np.asarray(x, np.float64).reshape(-1, 2); u = np.asarray(u, np.float64).reshape(-1, 2)
    p = np.concatenate([x, np.ones((len(x), 1))], 1)
    q = np.concatenate([u, np.zeros((len(x), 1))], 1) + np.cross(p, np.asarray(omega, np.float64)[None, :])
    ndp = p @ np.asarray(n, np.float64)
    with np.errstate(all="ignore"):
        if variant == SIM:
            a, b = ndp, np.full(len(x), float(d))
        else:
            a, b = np.ones(len(x)), float(d) / ndp
    return p, q, a, b


def kernel_sum(terms, index):
    """Sum of terms [m, k] whose rows are the kept points of point indices `index` (ascending), in the kernel's order: virtual wave
    vw and lane l add the points vw * 64 + l + 256 j in turn, each wave is reduced by the xor butterfly, the four as (0 + 1) + (2 + 3)."""
    terms = np.asarray(terms, np.float64)
    lanes = np.zeros((256,) + terms.shape[1:])
    for t, i in zip(terms, index):                              # ascending index: a lane meets its points in the kernel's order
        lanes[i % 256] += t
    part = []
    for vw in range(4):
        s = lanes[vw * 64:(vw + 1) * 64].copy()
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[np.arange(64) ^ o]
        part.append(s[0])
    return (part[0] + part[1]) + (part[2] + part[3])


def tri(C):
    return np.array([C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]])


def untri(t6):
    return np.array([[t6[0], t6[1], t6[2]], [t6[1], t6[3], t6[4]], [t6[2], t6[4], t6[5]]])


def _N(p):
    return np.sum(p * p, 1)[:, None, None] * np.eye(3)[None] - p[:, :, None] * p[:, None, :]


def _kept(x, valid, w):
    n = len(x)
    keep = np.ones(n, bool) if valid is None else np.asarray(valid).astype(bool).ravel()
    ww = np.ones(n) if w is None else np.asarray(w, np.float64).ravel()
    keep = keep & (ww > 0)
    return np.flatnonzero(keep), ww


def residual_ss(variant, x, u, d, n, omega, v, w):
    p, q, a, b = point_terms(variant, x, u, d, n, omega)
    r = a[:, None] * np.cross(p, np.asarray(v, np.float64)[None, :]) - b[:, None] * np.cross(p, q)
    return w * np.sum(r * r, 1)


def plain_solve(variant, x, u, d, n, omega, valid=None, w=None):
    """The (weighted) plain solve by the normal equations with the solve's rank rule: v, rss, rank."""
    x = np.asarray(x, np.float64).reshape(-1, 2); u = np.asarray(u, np.float64).reshape(-1, 2)
    idx, ww = _kept(x, valid, w)
    if not len(idx):
        return np.zeros(3), 0.0, 0
    p, q, a, b = point_terms(variant, x[idx], u[idx], d, n, omega)
    wk = ww[idx]
    pp = np.sum(p * p, 1)
    M = untri(kernel_sum((wk * a * a)[:, None] * np.stack([tri(m_) for m_ in _N(p)]), idx))
    Nq = pp[:, None] * q - p * np.sum(p * q, 1)[:, None]
    g = kernel_sum((wk * a * b)[:, None] * Nq, idx)
    if not (np.all(np.isfinite(M)) and np.all(np.isfinite(g))):
        return np.zeros(3), 0.0, 0
    lam, Q = np.linalg.eigh(M)
    lam = lam[::-1]; Q = Q[:, ::-1]
    tol = lam[0] * EPS * max(3.0 * len(idx), 3.0)
    v = np.zeros(3); rank = 0
    for k in range(3):
        if lam[k] > tol and lam[k] > 0:
            v += Q[:, k] * (Q[:, k] @ g) / lam[k]; rank += 1
    rss = float(kernel_sum(residual_ss(variant, x[idx], u[idx], d, n, omega, v, wk)[:, None], idx)[0])
    return v, rss, rank


def _sym_inverse(A, take):
    lam, Q = np.linalg.eigh(A)
    lam = lam[::-1]; Q = Q[:, ::-1]
    Ai = np.zeros((3, 3))
    for k in range(take):
        Ai += np.outer(Q[:, k], Q[:, k]) / lam[k]
    return Ai, lam


def joint_solve(variant, x, u, d, n, omega, sigma_flow, sigma_omega, v_s=None, rss_s=None, rank=None, valid=None, w=None, omega_var=None,
                usable=True):
    """One problem.  sigma_flow in the units of x and u; sigma_omega three values (inf: free, 0: held) or omega_var their variances.
    v_s, rss_s, rank: the solve's own outputs (None: plain_solve's).  Returns a dict: v, omega, rss (the record's fields after the joint
    solve), flag, rewritten (whether the record changes), rec (the 32 doubles), scale (the largest |b X q0| component, once the sums
    are formed)."""
    x = np.asarray(x, np.float64).reshape(-1, 2); u = np.asarray(u, np.float64).reshape(-1, 2)
    om = np.asarray(omega, np.float64)
    if v_s is None:
        v_s, rss_s, rank = plain_solve(variant, x, u, d, n, om, valid, w)
    v_s = np.asarray(v_s, np.float64)
    idx, ww = _kept(x, valid, w)
    m = len(idx)
    rec = np.zeros(JOINT_DOUBLES)
    rec[0:3] = om; rec[6:9] = v_s; rec[9] = rss_s; rec[10] = 1.0; rec[11] = m
    out = dict(v=v_s.copy(), omega=om.copy(), rss=rss_s, flag=1, rewritten=False, rec=rec)
    ovar = np.asarray(sigma_omega, np.float64) ** 2 if omega_var is None else np.asarray(omega_var, np.float64)
    ovar = np.broadcast_to(ovar, (3,)).astype(np.float64)
    dsf2 = (float(d) * float(sigma_flow)) ** 2
    if not usable or rank is None or rank < 3 or d == 0 or m == 0 or not np.isfinite(dsf2) or not np.all(np.isfinite(v_s)):
        return out
    p, q0, a, b = point_terms(variant, x[idx], u[idx], d, n, om)
    wk = ww[idx]
    pp = np.sum(p * p, 1)
    Nt = np.stack([tri(m_) for m_ in _N(p)])
    gk = wk * a * b * pp
    e = b[:, None] * q0 - a[:, None] * v_s[None, :]
    out["scale"] = float(np.abs(b[:, None] * np.cross(p, q0)).max())       # the size of a row's right-hand side: what a residual's rounding scales with
    with np.errstate(all="ignore"):
        sums = kernel_sum(np.concatenate([(wk * a * a)[:, None] * Nt, np.ones((m, 1)), np.stack([gk, gk * p[:, 0], gk * p[:, 1]], 1),
                                          (wk * b * b * pp)[:, None] * Nt, (wk * b * pp)[:, None] * np.cross(p, e)], 1), idx)
    if not np.all(np.isfinite(sums)):
        return out
    M = untri(sums[0:6]); D = untri(sums[10:16]); c = sums[16:19]
    K = -(sums[7] * skew([0, 0, 1.0]) + sums[8] * skew([1.0, 0, 0]) + sums[9] * skew([0, 1.0, 0]))     # X = skew(p), p = x e0 + y e1 + e2
    Mi, lam = _sym_inverse(M, 3)
    if not lam[2] > 0:
        return out
    G = Mi @ K
    held = ~(ovar > 0)
    est = np.flatnonzero(~held)
    S = D - K.T @ G
    S = 0.5 * (S + S.T)
    with np.errstate(all="ignore"):                              # a prior term that overflows is the header's "sum ... not finite"
        for k in est:
            if not np.isinf(ovar[k]):
                S[k, k] += dsf2 / ovar[k]
    S[held, :] = 0.0; S[:, held] = 0.0
    delta = np.zeros(3); Si = np.zeros((3, 3))
    if len(est):
        if not np.all(np.isfinite(S)):                           # flag 1, slots 12-14 left 0: joint_finish ends before the eigenvalues
            return out
        Si, ls = _sym_inverse(S, len(est))
        rec[12:15] = ls
        rec[12 + len(est):15] = 0.0                              # held axes: exact zeros on the device
        cut = np.sqrt(EPS * 3.0 * m) * ls[0]
        if np.any(~(ls[:len(est)] > 0)) or np.any(ls[:len(est)] < cut):
            rec[10] = 2.0; out["flag"] = 2
            return out
        delta = Si @ c
        delta[held] = 0.0
    v = v_s - G @ delta
    omh = om + delta
    if not (np.all(np.isfinite(v)) and np.all(np.isfinite(omh))):
        rec[12:15] = 0.0
        return out
    rec[0:3] = omh; rec[3:6] = delta; rec[10] = 0.0
    rec[15:21] = tri(dsf2 * Si); rec[21:27] = tri(dsf2 * (Mi + G @ Si @ G.T))
    out.update(flag=0, rec=rec)
    if len(est):
        rss = float(kernel_sum(residual_ss(variant, x[idx], u[idx], d, n, omh, v, wk)[:, None], idx)[0])
        out.update(v=v, omega=omh, rss=rss, rewritten=True)
    return out


def joint_lstsq(variant, x, u, d, n, omega, sigma_flow, sigma_omega, valid=None, w=None, scale_columns=False):
    """Independent: lstsq on the stacked rows sqrt(w) [a X, b N] (v, delta) = sqrt(w) b X q0 and the prior rows
    (d sigma_f / sigma_k) delta_k = 0; a held axis has no column.  scale_columns: every column is brought to unit length first (the
    unknowns rescaled, the problem unchanged), so that lstsq's rank cut, relative to the largest singular value, does not take v's
    columns for null beside a prior row of 1e150.  Returns v, omega."""
    x = np.asarray(x, np.float64).reshape(-1, 2); u = np.asarray(u, np.float64).reshape(-1, 2)
    om = np.asarray(omega, np.float64)
    idx, ww = _kept(x, valid, w)
    p, q0, a, b = point_terms(variant, x[idx], u[idx], d, n, om)
    sw = np.sqrt(ww[idx])
    X = np.stack([skew(pi) for pi in p])
    A = np.concatenate([(sw * a)[:, None, None] * X, (sw * b)[:, None, None] * _N(p)], 2).reshape(-1, 6)
    B = ((sw * b)[:, None] * np.einsum("nij,nj->ni", X, q0)).reshape(-1)
    so = np.broadcast_to(np.asarray(sigma_omega, np.float64), (3,))
    prior = np.zeros((3, 6))
    for k in range(3):
        if so[k] > 0 and np.isfinite(so[k]):
            prior[k, 3 + k] = float(d) * float(sigma_flow) / so[k]
    cols = [0, 1, 2] + [3 + k for k in range(3) if so[k] > 0]
    A = np.concatenate([A, prior], 0)[:, cols]
    B = np.concatenate([B, np.zeros(3)])
    cn = np.sqrt(np.sum(A * A, 0)) if scale_columns else np.ones(A.shape[1])
    sol = np.linalg.lstsq(A / cn, B, rcond=None)[0] / cn
    delta = np.zeros(3)
    delta[[c_ - 3 for c_ in cols[3:]]] = sol[3:]
    return sol[:3], om + delta


def rel_dev(v, omega, v_ref, omega_ref):
    """The deviation the tolerances are stated in: the larger of |v - v_ref| / |v_ref| and |omega - omega_ref| / |omega_ref|."""
    return max(np.linalg.norm(np.asarray(v) - v_ref) / np.linalg.norm(v_ref), np.linalg.norm(np.asarray(omega) - omega_ref) / np.linalg.norm(omega_ref))


# ---- the resident paths: one pair / one stream step from the points the device downloaded
def pair_joint(variant, prev, nxt, status, sr, sigma_flow_px, sigma_omega, rec, w=None, use_feas=False, feas_T=0.0, nrm=None, omega=None,
               omega_var=None, keep=None, solved=True):
    """The joint solve of one resident pair: prev / nxt [n,2] f32 (the points the solve stage read), status [n], sr the sensor row,
    rec the pair's record of a run with the setting OFF (v, RSS, rank).  Returns joint_solve's dict with v_uav added."""
    from oracle import estimation_oracle as eo
    d, scaling = sr[0], sr[19]
    nrm = sr[1:4] if nrm is None else nrm; omega = sr[4:7] if omega is None else omega
    new = np.asarray(nxt, np.float64); old = np.asarray(prev, np.float64)
    x = (new - [sr[20], sr[21]]) * scaling; u = (new - old) * scaling
    if keep is None:
        keep = np.asarray(status) == 1
        if use_feas and len(x):
            with np.errstate(all="ignore"):
                keep = keep & (eo.r_tilde(x, u, nrm, sr[22:25], d)[0] <= feas_T)
    out = joint_solve(variant, x, u, d, nrm, omega, sigma_flow_px * scaling, sigma_omega, v_s=rec[0:3], rss_s=rec[3], rank=rec[4], valid=keep,
                      w=w, omega_var=omega_var, usable=bool(solved) and scaling != 0)
    return out


# ---- the scenes the CPU and the GPU tests share
COUNTS = (3, 8, 63, 64, 65, 256, 257, 1025)
PRIORS = {"free": (np.inf, np.inf, np.inf), "prior": (1e-3, 1e-3, 1e-3), "mixed": (0.0, 1e-3, np.inf)}
SIGMA_FLOW = 2e-4                                               # 0.2 px at f = 1000
GYRO_ERROR = 3e-3 * np.array([1.0, -1.0, 0.5])


def scene(n, seed, noise=SIGMA_FLOW, outliers=False):
    """n points over a 1280 x 960 frame at f = 1000 (the first three spread wide, so that small n are well conditioned), the flow of
    (v, omega) over a slightly tilted plane with `noise` on it, and a gyro reading off by GYRO_ERROR.  outliers: every ninth point's
    flow is off by several sigma, for robust weights to find.  Returns x, u, d, nrm, omega0, v, omega."""
    from oracle import estimation_oracle as eo
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (n, 2)) * [0.64, 0.48]
    x[:3] = [[0.6, 0.45], [-0.6, -0.4], [0.55, -0.45]]
    nrm = np.array([0.05, -0.08, 1.0]); nrm /= np.linalg.norm(nrm)
    v = np.array([0.02, -0.015, 0.004]); om = np.array([0.004, -0.003, 0.01]); d = 1.5
    u = eo.generate_test_data(x, v, om, d, nrm)
    if noise:
        u = u + rng.normal(0, noise, u.shape)
    if outliers:
        u[5::9] += rng.normal(0, 20 * SIGMA_FLOW, u[5::9].shape)
    return x, u, d, nrm, om + GYRO_ERROR, v, om


def robust_weights(variant, x, u, d, nrm, omega0, valid=None, seed=5):
    """Final weights of tests/robust_reference.py's estimator (all ones below its minimum point count)."""
    import robust_reference as rr
    return rr.robust_solve(variant, x, u, d, nrm, omega0, valid=valid, loss=rr.TUKEY, hypotheses=16, seed=seed)["weights"]
