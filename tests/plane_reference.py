"""tests/plane_reference.py — numpy reference of the plane solve (ofk.h: ofk_set_plane; DESIGN.md "plane solve"): the ground normal
refined from the flow behind a velocity solve.

With p = (x, y, 1), X = [p]x, q = (u, 0) + p x omega, the solve's scalings sA, sB at the sensors' normal n0 and distance d0 (NODE:
sA = 1, sB = d0 / (n0.p); SIM: sA = n0.p, sB = d0) and m = n / d the plane's inverse-distance vector, point i's rows are
r_i = sB_i [(m.p_i) X_i v - X_i q_i]; at m0 = n0 / d0 they are the solve's.  The range along the beam e fixes the gauge: m = m0 + T tau
with T = [t1 t2] orthogonal to e.  The five unknowns (v, tau) come from a Gauss-Newton iteration started at the solve's v and tau = 0.

Two routes:
  plane_solve    the arithmetic of ofk.h restated: the 22 sums of every walk in the kernel's order (four virtual waves of 64 lanes, the
                 shuffle butterfly, (s0 + s1) + (s2 + s3)), the Schur complement step, the flags, the plane record.  M's inverse comes
                 from numpy's eigh, not from a cyclic Jacobi: close, not bit-identical, to the device.
  plane_lstsq    independent: Gauss-Newton where every step is np.linalg.lstsq on the stacked 3 m + 2 rows; no normal equations.
Nothing here imports the package: the tests feed it what the device downloaded."""
import numpy as np

from joint_reference import NODE, SIM, EPS, kernel_sum, point_terms, plain_solve, tri, untri, _N, _kept     # noqa: F401

PLANE_DOUBLES = 32
N_SUMS = 22


def beam_basis(beam):
    """e = beam / |beam|, T = [t1 t2]: t1 = normalize(e x a), a the coordinate axis of smallest |e_k| (lowest index on a tie),
    t2 = e x t1."""
    e = np.asarray(beam, np.float64)
    e = e / np.sqrt(e @ e)
    a = np.zeros(3); a[int(np.argmin(np.abs(e)))] = 1.0
    t1 = np.cross(e, a); t1 = t1 / np.sqrt(t1 @ t1)
    t2 = np.cross(e, t1)
    return e, np.stack([t1, t2], 1)


def walk_sums(p, q, sA, sB, wk, m, T, v, first, idx):
    """The 22 sums of one walk at (v, m): M 0-5, count 6, K 7-12 (row-major 3 x 2), D 13-15, g_v 16-18, g_tau 19-20, sum w |r|^2 21.
    In the first walk (tau = 0) the rows are the solve's own, a = sA; later a = sB (m.p)."""
    c = p @ m
    a = sA if first else sB * c
    y = np.cross(p, v[None, :])
    Xq = np.cross(p, q)
    r = a[:, None] * y - sB[:, None] * Xq
    h = p @ T
    z = -np.cross(p, y)                                         # X^T y
    Xtr = -np.cross(p, r)                                       # X^T r
    Nt = np.stack([tri(m_) for m_ in _N(p)])
    g = wk * sB * a
    terms = np.concatenate([
        (wk * a * a)[:, None] * Nt, np.ones((len(p), 1)),
        np.stack([g * z[:, 0] * h[:, 0], g * z[:, 0] * h[:, 1], g * z[:, 1] * h[:, 0], g * z[:, 1] * h[:, 1], g * z[:, 2] * h[:, 0],
                  g * z[:, 2] * h[:, 1]], 1),
        (wk * sB * sB * np.sum(y * y, 1))[:, None] * np.stack([h[:, 0] * h[:, 0], h[:, 0] * h[:, 1], h[:, 1] * h[:, 1]], 1),
        -(wk * a)[:, None] * Xtr,
        -(wk * sB * np.sum(y * r, 1))[:, None] * h,
        (wk * np.sum(r * r, 1))[:, None]], 1)
    return kernel_sum(terms, idx)


def sym2_inverse(a, b, c):
    """The symmetric 2 x 2 [[a, b], [b, c]] by its eigen-decomposition, in closed form: l1 >= l2 and the inverse (None where an
    eigenvalue is not positive)."""
    mean = 0.5 * (a + c)
    rad = np.sqrt((0.5 * (a - c)) ** 2 + b * b)
    l1 = mean + rad
    if not l1 > 0:
        return l1, 0.0, None
    l2 = (a * c - b * b) / l1
    if not l2 > 0:
        return l1, l2, None
    if b == 0:
        e1 = np.array([1.0, 0.0]) if a >= c else np.array([0.0, 1.0])
    else:
        e1 = np.array([l1 - c, b]) if a >= c else np.array([b, l1 - a])
        e1 = e1 / np.sqrt(e1 @ e1)
    e2 = np.array([-e1[1], e1[0]])
    return l1, l2, np.outer(e1, e1) / l1 + np.outer(e2, e2) / l2


def _m_inverse(M):
    lam, Q = np.linalg.eigh(M)
    lam = lam[::-1]; Q = Q[:, ::-1]
    if not lam[2] > 0:
        return None
    return sum(np.outer(Q[:, k], Q[:, k]) / lam[k] for k in range(3))


def rejected(f_final, f_first):
    """Flag 3's rule: the final objective is larger than the first walk's."""
    return bool(f_final > f_first)


def plane_solve(variant, x, u, d, n, omega, sigma_flow, sigma_normal, sigma_max=0.1, beam=(0.0, 0.0, 1.0), iters=6, v_s=None, rss_s=None,
                rank=None, valid=None, w=None, usable=True):
    """One problem.  sigma_flow in the units of x and u; sigma_normal in radians (inf: free, 0: held).  v_s, rss_s, rank: the solve's
    own outputs (None: plain_solve's).  Returns a dict: v, rss (the record's fields after the plane solve), flag, rewritten (whether the
    record changes), rec (the 32 doubles), m (the refined inverse-distance vector), scale (the largest |sB X q| component), cond (the
    condition number of the last walk's 5 x 5 system in the unknowns v / |v| and d0 tau), walks (the walks that were made), sigma (the
    predicted 1 sigma of the angle, once the last walk formed it: what sigma_max gates)."""
    x = np.asarray(x, np.float64).reshape(-1, 2); u = np.asarray(u, np.float64).reshape(-1, 2)
    n0 = np.asarray(n, np.float64); om = np.asarray(omega, np.float64)
    if v_s is None:
        v_s, rss_s, rank = plain_solve(variant, x, u, d, n0, om, valid, w)
    v_s = np.asarray(v_s, np.float64)
    idx, ww = _kept(x, valid, w)
    cnt = len(idx)
    d0 = float(d)
    rec = np.zeros(PLANE_DOUBLES)
    rec[0:3] = n0; rec[3] = d0; rec[6:9] = v_s; rec[9] = rss_s; rec[10] = 1.0; rec[11] = cnt
    out = dict(v=v_s.copy(), rss=rss_s, flag=1, rewritten=False, rec=rec, m=None)

    def flagged(f):
        rec[10] = float(f); out["flag"] = f
        rec[4:6] = 0.0; rec[14:26] = 0.0
        return out

    e, T = beam_basis(beam)
    dsf2 = (d0 * float(sigma_flow)) ** 2
    if (not usable or rank is None or rank < 3 or d0 == 0 or cnt == 0 or not np.isfinite(dsf2) or not np.all(np.isfinite(v_s))
            or not (n0 @ e != 0) or not np.isfinite(d0)):
        return out
    with np.errstate(all="ignore"):
        m0 = n0 / d0
        held = not sigma_normal > 0
        lroot = np.float64(0.0 if (held or np.isinf(sigma_normal)) else d0 * d0 * float(sigma_flow) / float(sigma_normal))
        lam = float(lroot * lroot)                              # a numpy scalar: a prior term that overflows is +inf, not an OverflowError
        if not np.isfinite(lam):                                # the header's "any sum or result is not finite": flag 1 before any sum is read
            return out
        p, q, sA, sB = point_terms(variant, x[idx], u[idx], d0, n0, om)
        out["scale"] = float(np.abs(sB[:, None] * np.cross(p, q)).max())
        wk = ww[idx]
        v = v_s.copy(); tau = np.zeros(2)
        f0 = step = 0.0
        for k in range(iters + 1):
            m = m0 + T @ tau
            s = walk_sums(p, q, sA, sB, wk, m, T, v, k == 0, idx)
            out["walks"] = k + 1
            if not np.all(np.isfinite(s)):
                return flagged(1)
            M = untri(s[0:6]); K = s[7:13].reshape(3, 2); gv = s[16:19]; gt = s[19:21]
            F = s[21] + lam * (tau @ tau)
            if k == 0:
                f0 = F; rec[26] = F
            Mi = _m_inverse(M)
            if Mi is None:
                return flagged(1)
            if held:                                            # nothing to estimate: the solve's record stands, C_v = (d sigma_f)^2 M^-1
                rec[0:3] = m0 / np.sqrt(m0 @ m0); rec[3] = 1.0 / np.sqrt(m0 @ m0)
                rec[10] = 0.0; rec[20:26] = tri(dsf2 * Mi); rec[27] = F
                out.update(flag=0, m=m0)
                return out
            G = Mi @ K
            S00 = s[13] + lam - K[:, 0] @ G[:, 0]; S01 = s[14] - K[:, 0] @ G[:, 1]; S11 = s[15] + lam - K[:, 1] @ G[:, 1]
            l1, l2, Si = sym2_inverse(S00, S01, S11)
            if not (np.isfinite(l1) and np.isfinite(l2)):
                return flagged(1)
            rec[12] = l1; rec[13] = l2
            if Si is None:
                return flagged(2)
            if k == iters:
                break
            dtau = Si @ (gt - lam * tau - K.T @ (Mi @ gv))
            dv = Mi @ (gv - K @ dtau)
            v = v + dv; tau = tau + dtau
            if not (np.all(np.isfinite(v)) and np.all(np.isfinite(tau))):
                return flagged(1)
            vn = np.sqrt(v @ v)
            step = np.sqrt(dv @ dv + d0 * d0 * (dtau @ dtau)) / vn if vn > 0 else 0.0
        rec[16] = step; rec[27] = F if np.isfinite(F) else 0.0
        sig = abs(d0) * np.sqrt(dsf2 / l2)
        out["sigma"] = float(sig)                               # the predicted 1 sigma, kept for the caller where the gate zeroes slot 14
        mm = np.sqrt(m @ m)
        nh = m / mm; dh = 1.0 / mm
        ang = np.arctan2(np.sqrt(np.sum(np.cross(nh, n0) ** 2)), nh @ n0)
        Cv = dsf2 * (Mi + G @ Si @ G.T)
        if not (np.isfinite(sig) and np.isfinite(F) and np.all(np.isfinite(nh)) and np.isfinite(dh) and np.isfinite(ang) and np.all(np.isfinite(Cv))
                and np.isfinite(step)):
            return flagged(1)
        if sig > sigma_max:
            return flagged(2)
        if rejected(F, f0):
            return flagged(3)
    rec[0:3] = nh; rec[3] = dh; rec[4:6] = tau; rec[10] = 0.0; rec[14] = sig; rec[15] = ang
    rec[17:20] = dsf2 * np.array([Si[0, 0], Si[0, 1], Si[1, 1]]); rec[20:26] = tri(Cv)
    H = np.block([[M, K], [K.T, np.array([[s[13] + lam, s[14]], [s[14], s[15] + lam]])]])
    vn = np.sqrt(v @ v)
    sc = np.diag([vn, vn, vn, 1.0 / d0, 1.0 / d0])              # the unknowns as relative quantities: v / |v| and the angle d0 tau
    out.update(v=v, rss=float(s[21]), flag=0, rewritten=True, m=m, cond=float(np.linalg.cond(sc @ H @ sc)))
    return out


def plane_lstsq(variant, x, u, d, n, omega, sigma_flow, sigma_normal, v_s, beam=(0.0, 0.0, 1.0), iters=6, valid=None, w=None):
    """Independent: `iters` Gauss-Newton steps from (v_s, 0), each np.linalg.lstsq on the stacked rows
    sqrt(w) sB [(m.p) X, (X v) h^T] (dv, dtau) = -sqrt(w) r and the prior rows sqrt(Lambda) dtau = -sqrt(Lambda) tau; a held tilt has
    no columns.  Returns v, m."""
    x = np.asarray(x, np.float64).reshape(-1, 2); u = np.asarray(u, np.float64).reshape(-1, 2)
    n0 = np.asarray(n, np.float64); d0 = float(d)
    idx, ww = _kept(x, valid, w)
    p, q, sA, sB = point_terms(variant, x[idx], u[idx], d0, n0, np.asarray(omega, np.float64))
    sw = np.sqrt(ww[idx])
    e, T = beam_basis(beam)
    held = not sigma_normal > 0
    sl = 0.0 if (held or np.isinf(sigma_normal)) else d0 * d0 * float(sigma_flow) / float(sigma_normal)
    X = np.zeros((len(p), 3, 3))
    X[:, 0, 1] = -p[:, 2]; X[:, 0, 2] = p[:, 1]; X[:, 1, 0] = p[:, 2]; X[:, 1, 2] = -p[:, 0]; X[:, 2, 0] = -p[:, 1]; X[:, 2, 1] = p[:, 0]
    Xq = np.einsum("nij,nj->ni", X, q)
    h = p @ T
    v = np.asarray(v_s, np.float64).copy(); tau = np.zeros(2)
    m0 = n0 / d0
    for _ in range(iters):
        m = m0 + T @ tau
        c = p @ m
        y = np.einsum("nij,j->ni", X, v)
        r = sB[:, None] * (c[:, None] * y - Xq)
        Jv = (sw * sB * c)[:, None, None] * X
        Jt = (sw * sB)[:, None, None] * y[:, :, None] * h[:, None, :]
        A = np.concatenate([Jv, Jt], 2).reshape(-1, 5)
        B = -(sw[:, None] * r).reshape(-1)
        A = np.concatenate([A, np.concatenate([np.zeros((2, 3)), sl * np.eye(2)], 1)], 0)
        B = np.concatenate([B, -sl * tau])
        if held:
            A = A[:-2, :3]; B = B[:-2]
        sol = np.linalg.lstsq(A, B, rcond=None)[0]
        v = v + sol[:3]
        if not held:
            tau = tau + sol[3:]
    return v, m0 + T @ tau


def rel_dev(v, m, v_ref, m_ref):
    """The deviation the tolerances are stated in: the larger of |v - v_ref| / |v_ref| and |m - m_ref| / |m_ref|."""
    return max(np.linalg.norm(np.asarray(v) - v_ref) / np.linalg.norm(v_ref), np.linalg.norm(np.asarray(m) - m_ref) / np.linalg.norm(m_ref))


def record_m(rec):
    """m^ = n^ / d^ of a plane record."""
    return np.asarray(rec[0:3], np.float64) / rec[3]


# ---- the resident paths: one pair / one stream step from the points the device downloaded
def pair_plane(variant, prev, nxt, status, sr, sigma_flow_px, sigma_normal, rec, sigma_max=0.1, beam=(0.0, 0.0, 1.0), iters=6, w=None,
               use_feas=False, feas_T=0.0, nrm=None, omega=None, keep=None, solved=True):
    """The plane solve of one resident pair: prev / nxt [n,2] f32 (the points the solve stage read), status [n], sr the sensor row,
    rec the pair's record of a run with the setting OFF (v, RSS, rank).  Returns plane_solve's dict."""
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
    return plane_solve(variant, x, u, d, nrm, omega, sigma_flow_px * scaling, sigma_normal, sigma_max, beam, iters, v_s=rec[0:3], rss_s=rec[3],
                       rank=rec[4], valid=keep, w=w, usable=bool(solved) and scaling != 0)


# ---- the scenes the CPU and the GPU tests share
COUNTS = (3, 8, 63, 64, 65, 256, 257, 1025)
PRIORS = {"free": np.inf, "prior": 0.05, "tight": 0.01}
SIGMA_FLOW = 2e-4                                               # 0.2 px at f = 1000
RANGE = 1.5                                                     # what the range sensor measured along the optical axis
SENSOR_NORMAL = np.array([np.sin(np.radians(2.0)), 0.0, np.cos(np.radians(2.0))])      # 2 degrees off a level plane


def rotate(a, axis, deg):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = np.radians(deg)
    return a * np.cos(t) + np.cross(axis, a) * np.sin(t) + axis * (axis @ a) * (1 - np.cos(t))


def scene(n, seed, slope_deg=10.0, noise=SIGMA_FLOW, outliers=False):
    """n points over a 1280 x 960 frame at f = 1000 (the first three spread wide, so that small n are well conditioned) and the flow of
    (v, omega) over a plane whose normal is `slope_deg` off the sensors' normal (itself 2 degrees off a level plane), with `noise` on
    it.  The range along the optical axis is RANGE for both, so d0 = (n0.e) RANGE and the true d = (n.e) RANGE.  outliers: every ninth
    point's flow is off by several sigma, for robust weights to find.  Returns x, u, d0, n0, omega, v, m_true."""
    from oracle import estimation_oracle as eo
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (n, 2)) * [0.64, 0.48]
    x[:3] = [[0.6, 0.45], [-0.6, -0.4], [0.55, -0.45]]
    n0 = SENSOR_NORMAL.copy()
    nt = rotate(n0, [0.3, 1.0, 0.0], slope_deg)
    v = np.array([0.02, -0.015, 0.004]); om = np.array([0.004, -0.003, 0.01])
    d0 = n0[2] * RANGE; dt = nt[2] * RANGE
    u = eo.generate_test_data(x, v, om, dt, nt)
    if noise:
        u = u + rng.normal(0, noise, u.shape)
    if outliers:
        u[5::9] += rng.normal(0, 20 * SIGMA_FLOW, u[5::9].shape)
    return x, u, d0, n0, om, v, nt / dt


def robust_weights(variant, x, u, d, nrm, omega0, valid=None, seed=5):
    """Final weights of tests/robust_reference.py's estimator (all ones below its minimum point count)."""
    import robust_reference as rr
    return rr.robust_solve(variant, x, u, d, nrm, omega0, valid=valid, loss=rr.TUKEY, hypotheses=16, seed=seed)["weights"]
