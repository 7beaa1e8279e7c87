"""tests/cov_reference.py — numpy reference of the velocity covariance (ofk.h: ofk_set_cov; DESIGN.md "velocity covariance").

First-order error propagation through the velocity solve.  With p = (x, y, 1), N(p) = |p|^2 I - p p^T = [p]x^T [p]x,
q = (u, 0) + p x omega and the per-point scalings a = sA, b = sB of the solve's variants (NODE: a = 1, b = d / (n.p); SIM: a = n.p,
b = d) the solve is v = M^+ g with M = sum w a^2 N, g = sum w a b N q.  For an input theta, dv = M^-1 sum_i e_i(theta),
    e_i = w [ (da b + a db) N q + a b (dN q + N dq) - 2 a da N v - a^2 dN v ],     dN r = 2 (p.dp) r - dp (p.r) - p (dp.r),
with the weights w held fixed.  Per direction:
    flow u_k      dq = e_k
    position x_k  dp = e_k, dq = e_k x omega, d(n.p) = n_k          (u held fixed)
    gyro omega_k  dq = p x e_k
    range d       db = 1 / (n.p) (NODE), 1 (SIM)
    normal n_k    d(n.p) = p_k
and d(n.p) enters as db = -d d(n.p) / (n.p)^2 (NODE) or da = d(n.p) (SIM).  Nothing here imports the package: the tests feed it what
the device downloaded.  oracle.estimation_oracle supplies the solve the finite-difference checks differentiate."""
import numpy as np

from oracle import estimation_oracle as eo

NODE, SIM = 0, 1
OFF, PROPAGATE, RESIDUAL = 0, 1, 2
COV_DOUBLES = 24
SIGMA_KEYS = ("sigma_flow", "sigma_pos", "sigma_d", "sigma_omega", "sigma_normal", "sigma_offset")     # ofk_cov's order
SHARE_KEYS = ("sigma_flow", "sigma_pos", "sigma_omega", "sigma_d", "sigma_normal", "sigma_offset")     # slots 16-21


def skew(a):
    a = np.asarray(a, np.float64)
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def _N(p, r):
    return np.sum(p * p, 1)[:, None] * r - p * np.sum(p * r, 1)[:, None]


def _dN(p, dp, r):
    return 2.0 * np.sum(p * dp, 1)[:, None] * r - dp * np.sum(p * r, 1)[:, None] - p * np.sum(dp * r, 1)[:, None]


def point_terms(variant, x, u, d, n, omega):
    x = np.asarray(x, np.float64)[:, :2]; u = np.asarray(u, np.float64)[:, :2]
    p = np.concatenate([x, np.ones((len(x), 1))], 1)
    q = np.concatenate([u, np.zeros((len(x), 1))], 1) + np.cross(p, np.asarray(omega, np.float64)[None, :])
    ndp = p @ np.asarray(n, np.float64)
    if variant == SIM:
        a, b = ndp, np.full(len(x), float(d))
    else:
        a, b = np.ones(len(x)), float(d) / ndp
    return p, q, a, b, ndp


def normal_equations(variant, x, u, d, n, omega, w=None):
    p, q, a, b, _ = point_terms(variant, x, u, d, n, omega)
    w = np.ones(len(p)) if w is None else np.asarray(w, np.float64)
    pp = np.sum(p * p, 1)
    M = np.einsum("i,ijk->jk", w * a * a, pp[:, None, None] * np.eye(3)[None] - p[:, :, None] * p[:, None, :])
    g = np.sum((w * a * b)[:, None] * _N(p, q), 0)
    return M, g


def _e(p, q, a, b, w, v, dp, dq, da, db):
    vv = np.broadcast_to(np.asarray(v, np.float64), p.shape)
    return w[:, None] * ((da * b + a * db)[:, None] * _N(p, q) + (a * b)[:, None] * (_dN(p, dp, q) + _N(p, dq))
                         - (2.0 * a * da)[:, None] * _N(p, vv) - (a * a)[:, None] * _dN(p, dp, vv))


def pre_vectors(variant, x, u, d, n, omega, v, w=None):
    """The per-point / summed vectors e before M^-1: flow [N,2,3], position [N,2,3], gyro [3,3] (row k: omega_k), range [3], normal [3,3]."""
    p, q, a, b, ndp = point_terms(variant, x, u, d, n, omega)
    N_ = len(p)
    w = np.ones(N_) if w is None else np.asarray(w, np.float64)
    om = np.asarray(omega, np.float64); n = np.asarray(n, np.float64)
    Z3 = np.zeros((N_, 3)); z = np.zeros(N_)
    unit = np.eye(3)

    def dndp(dn):                                               # d(n.p) -> (da, db)
        return (dn, z) if variant == SIM else (z, -float(d) * dn / (ndp * ndp))
    ef = np.zeros((N_, 2, 3)); ex = np.zeros((N_, 2, 3)); eg = np.zeros((3, 3)); en = np.zeros((3, 3))
    for k in range(2):
        ek = np.broadcast_to(unit[k], (N_, 3))
        ef[:, k] = _e(p, q, a, b, w, v, Z3, ek, z, z)
        da, db = dndp(np.full(N_, n[k]))
        ex[:, k] = _e(p, q, a, b, w, v, ek, np.broadcast_to(np.cross(unit[k], om), (N_, 3)), da, db)
    for k in range(3):
        eg[k] = _e(p, q, a, b, w, v, Z3, np.cross(p, unit[k][None, :]), z, z).sum(0)
        da, db = dndp(p[:, k])
        en[k] = _e(p, q, a, b, w, v, Z3, Z3, da, db).sum(0)
    ed = _e(p, q, a, b, w, v, Z3, Z3, z, np.ones(N_) if variant == SIM else 1.0 / ndp).sum(0)
    return ef, ex, eg, ed, en


def jacobians(variant, x, u, d, n, omega, t=None, w=None, v=None):
    """dv/d(input) of the plain solve (v = M^-1 g unless given): Ju [3,N,2], Jx [3,N,2], Jw [3,3] (with t: of v - omega x t, i.e.
    + [t]x), Jd [3], Jn [3,3], Jt [3,3] (= -[omega]x; zeros without t)."""
    M, g = normal_equations(variant, x, u, d, n, omega, w)
    Mi = np.linalg.inv(M)
    if v is None:
        v = Mi @ g
    ef, ex, eg, ed, en = pre_vectors(variant, x, u, d, n, omega, v, w)
    J = dict(Ju=np.einsum("jk,nck->jnc", Mi, ef), Jx=np.einsum("jk,nck->jnc", Mi, ex), Jw=Mi @ eg.T, Jd=Mi @ ed, Jn=Mi @ en.T,
             Jt=np.zeros((3, 3)), v=v, M=M, Minv=Mi)
    if t is not None:
        J["Jw"] = J["Jw"] + skew(t)
        J["Jt"] = -skew(omega)
    return J


def sigmas(**kw):
    s = dict(sigma_flow=0.0, sigma_pos=0.0, sigma_d=0.0, sigma_omega=(0.0, 0.0, 0.0), sigma_normal=0.0, sigma_offset=0.0)
    for k, val in kw.items():
        if k not in s:
            raise TypeError(k)
        s[k] = val
    if np.ndim(s["sigma_omega"]) == 0:
        s["sigma_omega"] = (float(s["sigma_omega"]),) * 3
    return s


def void_record():
    r = np.zeros(COV_DOUBLES); r[13] = 1.0
    return r


def tri(C):
    return np.array([C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]])


def untri(t6):
    return np.array([[t6[0], t6[1], t6[2]], [t6[1], t6[3], t6[4]], [t6[2], t6[4], t6[5]]])


def covariance(variant, x, u, d, n, omega, sig, mode=PROPAGATE, v=None, rss=None, rank=3, t=None, R=None, w=None, valid=None,
               omega_var=None):
    """The 24-double cov record of one problem.  v, rss, rank: the solve's own outputs (v before the lever arm; v None: M^-1 g and
    its residual).  t: lever arm / offset (None: none); R: rotation (None: I); w: robust weights over all points (0 = not kept);
    valid: mask over all points; omega_var: variances that replace sigma_omega^2 (the IMU state's slots 21-23)."""
    x = np.asarray(x, np.float64)[:, :2]; u = np.asarray(u, np.float64)[:, :2]
    keep = np.ones(len(x), bool) if valid is None else np.asarray(valid).astype(bool)
    ww = np.ones(len(x)) if w is None else np.asarray(w, np.float64)
    keep = keep & (ww > 0)
    x, u, ww = x[keep], u[keep], ww[keep]
    m = len(x)
    if m == 0 or rank < 3 or d == 0:
        return void_record()
    M, g = normal_equations(variant, x, u, d, n, omega, ww)
    lam = np.linalg.eigvalsh(M)
    if not np.all(np.isfinite(M)) or lam[0] <= 0:
        return void_record()
    Mi = np.linalg.inv(M)
    if v is None:
        v = Mi @ g
    v = np.asarray(v, np.float64)
    if rss is None:
        p, q, a, b, _ = point_terms(variant, x, u, d, n, omega)
        r = a[:, None] * np.cross(p, v[None, :]) - b[:, None] * np.cross(p, q)
        rss = float(np.sum(ww * np.sum(r * r, 1)))
    ef, ex, eg, ed, en = pre_vectors(variant, x, u, d, n, omega, v, ww)
    s2 = rss / (2 * m - 3) if 2 * m > 3 else 0.0
    if mode == RESIDUAL:
        if 2 * m <= 3:
            return void_record()
        Cf, Cx = s2 * Mi, np.zeros((3, 3))
    else:
        Cf = sig["sigma_flow"] ** 2 * Mi @ np.einsum("nck,ncl->kl", ef, ef) @ Mi
        Cx = sig["sigma_pos"] ** 2 * Mi @ np.einsum("nck,ncl->kl", ex, ex) @ Mi
    ov = np.asarray(sig["sigma_omega"], np.float64) ** 2 if omega_var is None else np.asarray(omega_var, np.float64)
    Jw = Mi @ eg.T
    Jd = Mi @ ed
    Jn = Mi @ en.T
    Cg = Jw @ np.diag(ov) @ Jw.T
    Cd = sig["sigma_d"] ** 2 * np.outer(Jd, Jd)
    Cn = sig["sigma_normal"] ** 2 * Jn @ Jn.T
    Cv = Cf + Cx + Cg + Cd + Cn
    if t is None:
        Cu, Cl = Cv.copy(), np.zeros((3, 3))
    else:
        Jwt = Jw + skew(t)
        W = skew(omega)
        Cl = sig["sigma_offset"] ** 2 * W @ W.T
        Cu = Cf + Cx + Jwt @ np.diag(ov) @ Jwt.T + Cd + Cn + Cl
    if R is not None:
        R = np.asarray(R, np.float64).reshape(3, 3)
        Cu = R @ Cu @ R.T
    rec = np.zeros(COV_DOUBLES)
    rec[0:6] = tri(Cv); rec[6:12] = tri(Cu); rec[12] = s2
    rec[16:22] = [np.trace(Cf), np.trace(Cx), np.trace(Cg), np.trace(Cd), np.trace(Cn), np.trace(Cl)]
    if not np.all(np.isfinite(rec)):
        return void_record()
    return rec


def predict_std(variant, x, u, d, n, omega, sig, t=None):
    """sqrt(diag(C_uav)) of a propagate-mode record: what a Monte-Carlo sweep's standard deviations estimate."""
    rec = covariance(variant, x, u, d, n, omega, sig, PROPAGATE, t=t)
    return np.sqrt(np.array([rec[6], rec[9], rec[11]]))


# ---- the filter step with R_eff, the innovation statistic and its gate
def r_eff(Rm, cov_rec, z_sign, z_source, r_floor):
    Rm = np.array(Rm, np.float64)
    if cov_rec is None or cov_rec[13] != 0.0:
        return Rm
    C = untri(cov_rec[6:12] if z_source else cov_rec[0:6])
    Re = Rm.copy()
    Re[:3, :3] = z_sign * z_sign * C + r_floor * np.eye(3)
    return Re


def kf_correct_cov(x, P, H, Rm, z, cov_rec=None, z_sign=1.0, z_source=0, filter_r=False, r_floor=0.0, nis_max=0.0):
    """One correct with R_eff (filter_r) or Rm: returns x, P, NIS, gated."""
    Re = r_eff(Rm, cov_rec, z_sign, z_source, r_floor) if filter_r else np.array(Rm, np.float64)
    nu = z - H @ x
    S = H @ P @ H.T + Re
    nis = float(nu @ np.linalg.solve(S, nu))
    if nis_max > 0 and nis > nis_max:
        return x, P, nis, 1.0
    x2, P2 = eo.kf_correct(x, P, H, Re, z)
    return x2, P2, nis, 0.0


# ---- the resident paths: one pair / one stream step from the points the device downloaded
def pair_record(variant, prev, nxt, status, sr, cfg, rec, w=None, use_feas=False, feas_T=0.0, nrm=None, omega=None, R=None, omega_var=None,
                keep=None):
    """The cov record of one resident pair: prev / nxt [n,2] f32 points, status [n], sr the sensor row (ofk.h), cfg a dict of
    mode, the six sigmas (sigma_flow / sigma_pos in pixels) and the filter fields, rec the pair's result record (v, RSS, rank).
    keep: the keep flags where the caller has them (a fused stream step); else status and the feasibility test.  nrm, omega, R:
    the IMU state's where it supplies them."""
    d, scaling = sr[0], sr[19]
    nrm = sr[1:4] if nrm is None else nrm; omega = sr[4:7] if omega is None else omega
    R = sr[7:16].reshape(3, 3) if R is None else np.asarray(R).reshape(3, 3)
    if scaling == 0 or d == 0:
        return void_record()
    new = np.asarray(nxt, np.float64); old = np.asarray(prev, np.float64)
    x = (new - [sr[20], sr[21]]) * scaling; u = (new - old) * scaling
    if keep is None:
        keep = np.asarray(status) == 1
        if use_feas and len(x):
            with np.errstate(all="ignore"):
                keep = keep & (eo.r_tilde(x, u, nrm, sr[22:25], d)[0] <= feas_T)
    sig = sigmas(sigma_flow=cfg["sigma_flow"] * scaling, sigma_pos=cfg["sigma_pos"] * scaling, sigma_d=cfg["sigma_d"],
                 sigma_omega=cfg["sigma_omega"], sigma_normal=cfg["sigma_normal"], sigma_offset=cfg["sigma_offset"])
    return covariance(variant, x, u, d, nrm, omega, sig, cfg["mode"], v=rec[0:3], rss=rec[3], rank=rec[4], t=sr[16:19], R=R, w=w, valid=keep,
                      omega_var=omega_var)


def condition(variant, prev, nxt, keep, sr, nrm=None, omega=None, w=None):
    """cond(M) of the kept points of a resident pair (the tests assert it is small: the rounding argument of the 1e-9 bound)."""
    new = np.asarray(nxt, np.float64)[keep]; old = np.asarray(prev, np.float64)[keep]
    x = (new - [sr[20], sr[21]]) * sr[19]; u = (new - old) * sr[19]
    M, _ = normal_equations(variant, x, u, sr[0], sr[1:4] if nrm is None else nrm, sr[4:7] if omega is None else omega,
                            None if w is None else np.asarray(w)[keep])
    return np.linalg.cond(M)


class CovStreamLoop:
    """The filter of one stream of ofk_stream_step_fused with a covariance setting on, in the style of tests/stream_oracle.py: per step
    predict with the control, the cov record from the step's points, then - on a solved step - the correct with R_eff, its NIS and
    the gate.  The image stages are not restated: the step is fed with the points, keep flags and sensors the device used."""

    def __init__(self, model, cfg, z_sign, z_source, variant=NODE):
        self.model, self.cfg, self.z_sign, self.z_source, self.variant = model, cfg, z_sign, z_source, variant
        self.x, self.P = np.array(model.x0, np.float64), np.array(model.P0, np.float64)

    def step(self, old, new, keep, sr, rec, control, imu=None, w=None):
        """old / new [n,2] f32; keep [n]; sr the sensor row; rec the step's result record; control the filter's input; imu: the resident
        IMU state row (normal, omega, rotation, angular-velocity variances) when the fusion reads it.  Returns the cov record
        (NIS, gated filled in), x, P, fused [8]."""
        m, cfg = self.model, self.cfg
        self.x, self.P = eo.kf_predict(self.x, self.P, m.F, m.Q, m.B if m.nc else None, np.asarray(control, np.float64) if m.nc else None)
        kw = {}
        if imu is not None:
            kw = dict(nrm=imu[15:18], omega=imu[18:21], R=imu[6:15], omega_var=imu[21:24] if cfg.get("omega_from_imu") else None)
        cv = pair_record(self.variant, old, new, None, sr, cfg, rec, w=w, keep=np.asarray(keep).astype(bool), **kw)
        solved = rec[15] != 0
        if solved:
            z = self.z_sign * np.asarray(rec[8:11] if self.z_source else rec[0:3], np.float64)
            if m.nm > 3:
                z = np.concatenate([z, sr[22:22 + m.nm - 3]])
            self.x, self.P, cv[14], cv[15] = kf_correct_cov(self.x, self.P, m.H, m.R, z, cov_rec=cv, z_sign=self.z_sign, z_source=self.z_source,
                                                            filter_r=bool(cfg.get("filter_r")), r_floor=cfg.get("r_floor", 0.0),
                                                            nis_max=cfg.get("nis_max", 0.0))
        fused = np.zeros(8)
        fused[:m.ns] = self.x; fused[6] = np.trace(self.P); fused[7] = 1.0 if solved else 0.0
        return cv, self.x.copy(), self.P.copy(), fused
