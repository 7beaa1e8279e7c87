"""tests/epi_reference.py — numpy reference of the epipolar solve (ofk.h: ofk_set_epipolar; DESIGN.md "epipolar solve").

With p = (x, y, 1), X = [p]x and q = (u, 0) + p x omega the flow equation is rho_i X v = X q_i, rho_i point i's inverse depth.
c_i = p_i x q_i is orthogonal to v whatever rho_i is; flow noise enters c_i as X_i (delta, 0), so E = sum w c c^T has the expectation
E0 + sigma^2 N0, N0 = sum w X D X^T, and t^ is the generalised eigenvector of (E, N0) for the smallest eigenvalue.  The scale comes
from the range: over the anchor set around the beam's foot kappa_i = s m_i, m_i = (n0.p_i) / d0.

Two routes:
  epi_solve        the arithmetic of ofk.h restated: the 13 + 15 sums in the kernel's order (four virtual waves of 64 lanes, the
                   shuffle butterfly, (s0 + s1) + (s2 + s3)), W = N0^(-1/2), the smallest eigenvector of W E W, sign, gate, scale,
                   the flags, the record and the point rows.  The 3 x 3 eigen-decompositions come from numpy's eigh, not from a
                   cyclic Jacobi: close, not bit-identical, to the device.
  epi_independent  independent: plain numpy sums, a Cholesky factor of N0 in the place of its inverse square root, eigh on the
                   whitened matrix, np.linalg.lstsq for s.
Nothing here imports the package: the tests feed it what the device downloaded."""
import numpy as np

from joint_reference import EPS, NODE, SIM, kernel_sum, plain_solve, point_terms, tri, untri  # noqa: F401

EPI_DOUBLES = 32
W_ONE, W_ROBUST = 0, 1


def flow(x, v, omega, rho):
    """The instantaneous flow of points x [n,2] at inverse depths rho [n] under (v, omega): rho (v - v_z p) + omega x p - (omega x p)_z p."""
    x = np.asarray(x, np.float64).reshape(-1, 2)
    p = np.concatenate([x, np.ones((len(x), 1))], 1)
    v = np.asarray(v, np.float64)
    wxp = np.cross(np.asarray(omega, np.float64)[None, :], p)
    f = np.asarray(rho, np.float64)[:, None] * (v[None, :] - v[2] * p) + (wxp - wxp[:, 2:3] * p)
    return f[:, :2]


def plane_rho(x, d, n):
    x = np.asarray(x, np.float64).reshape(-1, 2)
    return (x @ np.asarray(n, np.float64)[:2] + n[2]) / float(d)


def _kept(x, valid, w, weights):
    n = len(x)
    keep = np.ones(n, bool) if valid is None else np.asarray(valid).astype(bool).ravel()
    ww = np.ones(n)
    if weights == W_ROBUST and w is not None:
        ww = np.asarray(w, np.float64).ravel().copy()
        keep = keep & (ww > 0)
    return keep, ww


def _sum(terms, idx, fast):
    return np.sum(terms, 0) if fast else kernel_sum(terms, idx)


def _outer6(c):
    return np.stack([c[:, 0] * c[:, 0], c[:, 0] * c[:, 1], c[:, 0] * c[:, 2], c[:, 1] * c[:, 1], c[:, 1] * c[:, 2], c[:, 2] * c[:, 2]], 1)


def _eigh_desc(A):
    lam, Q = np.linalg.eigh(A)
    return lam[::-1], Q[:, ::-1]


def epi_solve(x, u, d, n, omega, anchor=np.inf, anchor_min=5, sigma_max=np.inf, beam=(0.0, 0.0, 1.0), weights=W_ONE, v_s=None, rss_s=None,
              valid=None, w=None, usable=True, fast=False):
    """One problem.  anchor in the units of x.  v_s, rss_s: fields 0-3 of the solve's record before (None: the plain NODE solve's).
    fast: plain numpy sums in the place of the kernel's order (for statistics over many problems).
    Returns a dict: v, rss (the record's fields 0-3 after), t, s, sigma, pred, flag, rewritten, rec (the 32 doubles), rows [n,4],
    rho [kept], a_max (the largest |a_i|: what a point's r rounds with)."""
    x = np.asarray(x, np.float64).reshape(-1, 2); u = np.asarray(u, np.float64).reshape(-1, 2)
    om = np.asarray(omega, np.float64); nrm = np.asarray(n, np.float64)
    if v_s is None:
        v_s, rss_s, _ = plain_solve(NODE, x, u, d, nrm, om, valid, w if weights == W_ROBUST else None)
    v_s = np.asarray(v_s, np.float64)
    keep, ww = _kept(x, valid, w, weights)
    idx = np.flatnonzero(keep)
    m = len(idx)
    rec = np.zeros(EPI_DOUBLES)
    rec[6:9] = v_s; rec[9] = rss_s; rec[10] = 1.0; rec[11] = m
    rows = np.zeros((len(x), 4))
    out = dict(v=v_s.copy(), rss=rss_s, t=np.zeros(3), s=0.0, sigma=0.0, pred=0.0, flag=1, rewritten=False, rec=rec, rows=rows, rho=np.zeros(0), a_max=0.0)
    e = np.asarray(beam, np.float64); e = e / np.linalg.norm(e)
    d = float(d)
    ne = float(nrm @ e)
    if not usable or not np.isfinite(d) or d == 0 or not np.isfinite(ne) or ne == 0 or e[2] == 0 or m < 3:
        return out
    p, q, _, _ = point_terms(NODE, x[idx], u[idx], 1.0, np.array([0.0, 0.0, 1.0]), om)
    wk = ww[idx]
    c = np.cross(p, q)
    px, py = p[:, 0], p[:, 1]
    N6 = np.stack([np.ones(m), np.zeros(m), -px, np.ones(m), -py, px * px + py * py], 1)
    with np.errstate(all="ignore"):
        s1 = _sum(np.concatenate([wk[:, None] * _outer6(c), wk[:, None] * N6, np.ones((m, 1))], 1), idx, fast)
    if not np.all(np.isfinite(s1)):
        return out
    E = untri(s1[0:6]); N0 = untri(s1[6:12])
    ln, Vn = _eigh_desc(N0)
    if not (ln[2] > EPS * 3.0 * m * ln[0]):
        return out
    W = (Vn / np.sqrt(ln)[None, :]) @ Vn.T
    G = W @ E @ W
    lg, Y = _eigh_desc(0.5 * (G + G.T))
    th = W @ Y[:, 2]
    nn = np.linalg.norm(th)
    if not (np.all(np.isfinite(lg)) and np.isfinite(nn) and nn > 0):
        return out
    t = th / nn
    tnt = 1.0 / (nn * nn)                                       # t^^T N0 t^: W N0 W = I and |y| = 1
    rec[14:16] = lg[:2]
    # second walk
    a = q[:, :2] - q[:, 2:3] * p[:, :2]
    b = t[None, :2] - t[2] * p[:, :2]
    with np.errstate(all="ignore"):
        bb = np.sum(b * b, 1); ab = np.sum(a * b, 1); nb = np.sqrt(bb)
        kap = ab / bb
        cr = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        r = cr / nb
        mi = (p @ nrm) / d
        pe = e[:2] / e[2]
        inA = (np.sum((p[:, :2] - pe[None, :]) ** 2, 1) <= float(anchor) ** 2).astype(np.float64)
        wb = wk / bb
        s2 = _sum(np.concatenate([wb[:, None] * _outer6(c), (wk * r * r)[:, None], (wk * ab)[:, None],
                                  np.where(inA > 0, wk * kap * mi, 0.0)[:, None], np.where(inA > 0, wk * mi * mi, 0.0)[:, None],
                                  np.where(inA > 0, wb * mi * mi, 0.0)[:, None], inA[:, None], (kap <= 0)[:, None] * 1.0, (kap >= 0)[:, None] * 1.0,
                                  (wk * cr * cr)[:, None]], 1), idx, fast)
    out["a_max"] = float(np.sqrt(np.sum(a * a, 1)).max())
    if not np.all(np.isfinite(s2)):
        rec[14:16] = 0.0
        return out
    sgn = 1.0 if s2[7] >= 0 else -1.0
    l1 = s2[14] / tnt                                           # lambda_1 as t^'s Rayleigh quotient, from residuals
    sig2 = l1 * m / (m - 2.0)
    rec[4] = np.sqrt(sig2); rec[16] = l1
    t = sgn * t
    rec[0:3] = t; rec[5] = s2[6]; rec[12] = s2[11]; rec[13] = s2[12] if sgn > 0 else s2[13]
    out.update(t=t.copy(), sigma=float(rec[4]))
    H = untri(s2[0:6]); P = np.eye(3) - np.outer(t, t)
    PHP = P @ H @ P
    lh, Vh = _eigh_desc(0.5 * (PHP + PHP.T))
    if not (lh[1] > 0 and np.isfinite(lh[0])):
        rec[17] = np.inf; rec[10] = 2.0
        out.update(flag=2, pred=np.inf)
        return out
    Ct = sig2 * (np.outer(Vh[:, 0], Vh[:, 0]) / lh[0] + np.outer(Vh[:, 1], Vh[:, 1]) / lh[1])
    pred = float(np.sqrt(np.trace(Ct)))
    rec[17] = pred
    out["pred"] = pred
    if not (pred <= sigma_max):
        rec[10] = 2.0; out["flag"] = 2
        return out
    rec[18:24] = tri(Ct)
    with np.errstate(all="ignore"):
        sraw = s2[8] / s2[9]
    sc = sgn * sraw
    if s2[11] < anchor_min or not (np.isfinite(sc) and sc > 0):
        rec[10] = 3.0; out["flag"] = 3
        return out
    vs = sig2 * s2[10] / (s2[9] * s2[9])
    rec[3] = sc; rec[24] = vs; rec[10] = 0.0
    v = sc * t
    rec[25:31] = tri(sc * sc * Ct + vs * np.outer(t, t))
    rows[~keep, 3] = 1.0
    rows[idx, 0] = kap / sraw; rows[idx, 1] = sgn * r; rows[idx, 2] = nb; rows[idx, 3] = np.where(sgn * kap <= 0, 2.0, 0.0)
    out.update(v=v, rss=float(s2[6]), s=float(sc), flag=0, rewritten=True, rho=kap / sraw)
    return out


def epi_independent(x, u, d, n, omega, anchor=np.inf, beam=(0.0, 0.0, 1.0), valid=None, w=None, weights=W_ONE):
    """Independent: t^ from eigh on L^-1 E L^-T, N0 = L L^T (Cholesky), s from np.linalg.lstsq over the anchor set.  Returns t^, s."""
    x = np.asarray(x, np.float64).reshape(-1, 2); u = np.asarray(u, np.float64).reshape(-1, 2)
    keep, ww = _kept(x, valid, w, weights)
    idx = np.flatnonzero(keep)
    p = np.concatenate([x[idx], np.ones((len(idx), 1))], 1)
    q = np.concatenate([u[idx], np.zeros((len(idx), 1))], 1) + np.cross(p, np.asarray(omega, np.float64)[None, :])
    wk = ww[idx]
    c = np.cross(p, q)
    E = np.einsum("n,ni,nj->ij", wk, c, c)
    D = np.diag([1.0, 1.0, 0.0])
    N0 = np.zeros((3, 3))
    for wi, pi in zip(wk, p):
        X = np.array([[0.0, -pi[2], pi[1]], [pi[2], 0.0, -pi[0]], [-pi[1], pi[0], 0.0]])
        N0 += wi * X @ D @ X.T
    L = np.linalg.cholesky(N0)
    Li = np.linalg.inv(L)
    A = Li @ E @ Li.T
    lam, Z = np.linalg.eigh(0.5 * (A + A.T))
    t = Li.T @ Z[:, 0]
    t /= np.linalg.norm(t)
    a = q[:, :2] - q[:, 2:3] * p[:, :2]
    b = t[None, :2] - t[2] * p[:, :2]
    if np.sum(wk * np.sum(a * b, 1)) < 0:
        t = -t; b = -b
    kap = np.sum(a * b, 1) / np.sum(b * b, 1)
    e = np.asarray(beam, np.float64); e = e / np.linalg.norm(e)
    inA = np.sum((p[:, :2] - (e[:2] / e[2])[None, :]) ** 2, 1) <= float(anchor) ** 2
    mi = (p @ np.asarray(n, np.float64)) / float(d)
    sw = np.sqrt(wk[inA])
    s = np.linalg.lstsq((sw * mi[inA])[:, None], sw * kap[inA], rcond=None)[0][0]
    return t, float(s)


def rel_dev(t, s, t_ref, s_ref):
    """The deviation the tolerances are stated in: the larger of |t^ - t^_ref| (unit vectors) and |s - s_ref| / |s_ref|."""
    return max(float(np.linalg.norm(np.asarray(t) - t_ref)), abs(s - s_ref) / abs(s_ref))


def rows_dev(rows, ref, a_max):
    """The point rows' deviations in the same spirit: rho and |b| relative to the largest |rho| and |b| of the reference, r relative to
    the largest derotated flow |a_i| (r is a residual: it rounds with the flow it is the difference of).  Flags must agree."""
    rows = np.asarray(rows); ref = np.asarray(ref)
    assert np.array_equal(rows[:, 3], ref[:, 3]), "point flags differ"
    dr = np.abs(rows[:, 0] - ref[:, 0]).max() / max(np.abs(ref[:, 0]).max(), 1e-300)
    db = np.abs(rows[:, 2] - ref[:, 2]).max() / max(np.abs(ref[:, 2]).max(), 1e-300)
    return max(dr, db), np.abs(rows[:, 1] - ref[:, 1]).max() / max(a_max, 1e-300)


def record_scale(rec):
    """Per-slot scales of a record for the 1e-9 comparison: a slot group is compared relative to its own largest magnitude."""
    rec = np.asarray(rec, np.float64)
    sc = np.ones(EPI_DOUBLES)
    for lo, hi in ((0, 3), (3, 4), (4, 5), (5, 6), (6, 9), (9, 10), (14, 17), (17, 18), (18, 24), (24, 25), (25, 31)):
        g = np.abs(rec[lo:hi]); g = g[np.isfinite(g)]
        sc[lo:hi] = max(g.max() if len(g) else 0.0, 1e-300)
    sc[5] = max(sc[5], sc[14])                                  # sum w r^2 and lambda_1 are sums of squared residuals: they round with E
    sc[16] = sc[14]
    return sc


# ---- the resident paths: one pair / one stream step from the points the device downloaded
def pair_epi(prev, nxt, status, sr, rec, anchor_px=np.inf, anchor_min=5, sigma_max=np.inf, beam=(0.0, 0.0, 1.0), weights=W_ONE, w=None,
             use_feas=False, feas_T=0.0, nrm=None, omega=None, keep=None, solved=True):
    """The epipolar solve of one resident pair: prev / nxt [n,2] f32 (the points the solve stage read), status [n], sr the sensor row,
    rec the pair's record of a run with the setting OFF.  Returns epi_solve's dict."""
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
    return epi_solve(x, u, d, nrm, omega, anchor_px * scaling, anchor_min, sigma_max, beam, weights, v_s=rec[0:3], rss_s=rec[3], valid=keep, w=w,
                     usable=bool(solved) and scaling != 0 and np.isfinite(scaling))


# ---- the scenes the CPU and the GPU tests share
COUNTS = (3, 4, 63, 64, 65, 255, 256, 257, 1025)
V, OM, D = np.array([0.02, -0.015, 0.004]), np.array([0.004, -0.003, 0.01]), 1.5
NRM = np.array([0.0, 0.0, 1.0])
SIGMA_FLOW = 2e-4                                               # 0.2 px at f = 1000
FOOT = 0.12                                                     # the ground inside this radius of the beam's foot stays level


def points(n, rng):
    """n points over a 1280 x 960 frame at f = 1000; the first three spread wide (small n stay well conditioned) and, from 8 points on,
    five more inside the foot, so that the default anchor_min is met at every count the tests use."""
    x = rng.uniform(-1.0, 1.0, (n, 2)) * [0.64, 0.48]
    x[:3] = [[0.6, 0.45], [-0.6, -0.4], [0.55, -0.45]]
    if n >= 8:
        x[3:8] = [[0.05, 0.02], [-0.06, 0.04], [0.02, -0.07], [-0.03, -0.05], [0.08, -0.01]]
    return x


def relief(kind, x, rng):
    """Relief h of the four scenes of the experiment (Z = Z_plane (1 - h), level inside FOOT of the optical axis)."""
    n = len(x)
    h = np.zeros(n)
    if kind == "block30":
        h[x[:, 0] > 0.64 - 0.3 * 1.28] = 0.3
    elif kind == "block60":
        h[x[:, 0] > 0.64 - 0.6 * 1.28] = 0.3
    elif kind == "canopy":
        up = rng.uniform(size=n) < 0.6
        h[up] = rng.uniform(0.1, 0.5, int(up.sum()))
    elif kind == "ramp":
        h = 0.35 * (x[:, 0] + 0.64) / 1.28
    elif kind != "flat":
        raise ValueError(kind)
    h[np.hypot(x[:, 0], x[:, 1]) <= FOOT] = 0.0
    return h


def scene(n, seed, kind="canopy", noise=SIGMA_FLOW, outliers=False, v=V, omega=OM):
    """n points, the flow of (v, omega) over ground with relief `kind` and `noise` on it.  outliers: every ninth point's flow is off by
    several sigma, for robust weights to find.  Returns x, u, d, nrm, omega, v, rho."""
    rng = np.random.default_rng(seed)
    x = points(n, rng)
    rho = plane_rho(x, D, NRM) / (1.0 - relief(kind, x, rng))
    u = flow(x, v, omega, rho)
    if noise:
        u = u + rng.normal(0, noise, u.shape)
    if outliers:
        u[5::9] += rng.normal(0, 20 * SIGMA_FLOW, u[5::9].shape)
    return x, u, D, NRM.copy(), np.asarray(omega, np.float64).copy(), np.asarray(v, np.float64).copy(), rho


def robust_weights(x, u, d, nrm, omega, valid=None, seed=5):
    """Final weights of tests/robust_reference.py's estimator (all ones below its minimum point count)."""
    import robust_reference as rr
    return rr.robust_solve(NODE, x, u, d, nrm, omega, valid=valid, loss=rr.TUKEY, hypotheses=16, seed=seed)["weights"]
