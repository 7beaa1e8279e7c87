"""The position filter of a stream (include/ofk.h: ofk_set_pos_filter) restated in numpy, rule by rule and in the header's order of
operations, plus the scenario generator of the experiment behind the README's figures.  One stream per call; f64 throughout."""
import numpy as np

N, INPUT, INTS, DOUBLES = 12, 12, 16, 48
NOT, APPLIED, GATED, REFUSED = 0, 1, 2, 3
KEY_SOLVED = 0
DEFAULTS = dict(dt=1.0, sigma_v=1e-3, floor=0.0, infl=1.0, share=0.5, q_p=0.0, q_v=1e-3, q_b=0.0, p0_p=0.0, p0_v=1.0, p0_b=0.0, nis_max=0.0)


def setting(**kw):
    s = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in s:
            raise TypeError(k)
        s[k] = float(v)
    return s


def _same(cond):
    """A decision of the rules over the leading axes: every stream of one call must take the same path."""
    c = np.asarray(cond)
    if c.all():
        return True
    if not c.any():
        return False
    raise ValueError("the streams of one call must take the same path through the rules")


def new_state(pos=(0.0, 0.0, 0.0), lead=()):
    """What k_pos_filter_clear leaves: not started, at pos.  lead: leading axes (streams in lockstep)."""
    x = np.zeros(tuple(lead) + (N,))
    x[..., 0:3] = pos
    x[..., 9:12] = pos
    ist = np.zeros(INTS, np.int32)                               # shared: the streams of one state take the same path
    ist[1] = 1
    return dict(x=x, P=np.zeros(tuple(lead) + (N, N)), istate=ist)


def start(st, s):
    """Rule 1."""
    x, P = st["x"], st["P"]
    p = x[..., 0:3].copy()
    x[:] = 0.0
    x[..., 0:3] = p
    x[..., 9:12] = p
    P[:] = 0.0
    for k in range(3):
        for a in (0, 9):
            for c in (0, 9):
                P[..., a + k, c + k] = s["p0_p"] * s["p0_p"]
        P[..., 3 + k, 3 + k] = s["p0_v"] * s["p0_v"]
        P[..., 6 + k, 6 + k] = s["p0_b"] * s["p0_b"]
    st["istate"][1] = 1
    st["istate"][3] = 1


def predict(st, s, du):
    """Rule 2."""
    x, P, dt = st["x"], st["P"], s["dt"]
    du = np.where(np.isfinite(du), du, 0.0)
    xn = x.copy()
    xn[..., 0:3] = x[..., 0:3] + dt * x[..., 3:6]
    xn[..., 3:6] = (x[..., 3:6] + du) - dt * x[..., 6:9]
    G = P.copy()                                                 # G_ij = P_ij + f_i P_i+3,j
    G[..., 0:3, :] = P[..., 0:3, :] + dt * P[..., 3:6, :]
    G[..., 3:6, :] = P[..., 3:6, :] + (-dt) * P[..., 6:9, :]
    Pn = G.copy()                                                # P'_ij = G_ij + f_j G_i,j+3
    Pn[..., :, 0:3] = G[..., :, 0:3] + dt * G[..., :, 3:6]
    Pn[..., :, 3:6] = G[..., :, 3:6] + (-dt) * G[..., :, 6:9]
    q = np.array([s["q_p"]] * 3 + [s["q_v"]] * 3 + [s["q_b"]] * 3 + [0.0] * 3)
    d = np.arange(N)
    Pn[..., d, d] = Pn[..., d, d] + q * q
    x[:] = xn
    P[:] = Pn


def s_matrix(P, ia, ic, R):
    S = np.empty(P.shape[:-2] + (3, 3))
    for m in range(3):
        for n in range(3):
            h = P[..., ia + m, ia + n] if ic is None else \
                ((P[..., ia + m, ia + n] - P[..., ia + m, ic + n]) - P[..., ic + m, ia + n]) + P[..., ic + m, ic + n]
            S[..., m, n] = h + R[..., m, n]
    return S


TINY = 2.0 ** -48                                               # 16 ulp of 1


def pivot_scale(P, ia, ic, m):
    """What pivot m of S was formed from: a pivot not above TINY times this is rounding noise of its own terms."""
    a = np.abs(P[..., ia + m, ia + m])
    return a if ic is None else ((a + np.abs(P[..., ia + m, ic + m])) + np.abs(P[..., ic + m, ia + m])) + np.abs(P[..., ic + m, ic + m])


def update(st, ia, ic, z, R, nis_max):
    """Rule 6 -> (outcome, NIS, y).  ia: the block of +I, ic: the block of -I or None."""
    x, P = st["x"], st["P"]
    z = np.asarray(z, np.float64); R = np.asarray(R, np.float64)
    S = s_matrix(P, ia, ic, R)
    tiny = [TINY * pivot_scale(P, ia, ic, m) for m in range(3)]
    y = z - x[..., ia:ia + 3] if ic is None else z - (x[..., ia:ia + 3] - x[..., ic:ic + 3])
    zero = np.zeros(y.shape[:-1])
    with np.errstate(all="ignore"):
        d0 = S[..., 0, 0]
        if not _same(np.isfinite(d0) & (d0 > tiny[0])):
            return REFUSED, zero, y
        l00 = np.sqrt(d0); l10 = S[..., 1, 0] / l00; l20 = S[..., 2, 0] / l00
        d1 = S[..., 1, 1] - l10 * l10
        if not _same(np.isfinite(d1) & (d1 > tiny[1])):
            return REFUSED, zero, y
        l11 = np.sqrt(d1); l21 = (S[..., 2, 1] - l20 * l10) / l11
        d2 = (S[..., 2, 2] - l20 * l20) - l21 * l21
        if not _same(np.isfinite(d2) & (d2 > tiny[2])):
            return REFUSED, zero, y
        l22 = np.sqrt(d2)

        def forward(a0, a1, a2):
            t0 = a0 / l00
            t1 = (a1 - l10 * t0) / l11
            t2 = ((a2 - l20 * t0) - l21 * t1) / l22
            return t0, t1, t2
        w = forward(y[..., 0], y[..., 1], y[..., 2])
        nis = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
        if not _same(np.isfinite(nis)):
            return REFUSED, zero, y
        if nis_max > 0.0 and _same(nis > nis_max):
            return GATED, nis, y
        if ic is None:
            PHt = P[..., :, ia:ia + 3].copy(); HP = P[..., ia:ia + 3, :].copy()
        else:
            PHt = P[..., :, ia:ia + 3] - P[..., :, ic:ic + 3]; HP = P[..., ia:ia + 3, :] - P[..., ic:ic + 3, :]
        e = lambda a: a[..., None]                               # a factor per stream against the rows of a strip
        L00, L10, L20, L11, L21, L22 = e(l00), e(l10), e(l20), e(l11), e(l21), e(l22)
        t0 = PHt[..., 0] / L00                                   # row i of K solves S k = (P H^T)_i
        t1 = (PHt[..., 1] - L10 * t0) / L11
        t2 = ((PHt[..., 2] - L20 * t0) - L21 * t1) / L22
        k2 = t2 / L22
        k1 = (t1 - L21 * k2) / L11
        k0 = ((t0 - L10 * k1) - L20 * k2) / L00
        K = np.stack([k0, k1, k2], axis=-1)
        x[:] = x + ((K[..., 0] * y[..., 0:1] + K[..., 1] * y[..., 1:2]) + K[..., 2] * y[..., 2:3])
        B = P - ((K[..., :, 0:1] * HP[..., 0:1, :] + K[..., :, 1:2] * HP[..., 1:2, :]) + K[..., :, 2:3] * HP[..., 2:3, :])
        BHt = B[..., :, ia:ia + 3].copy() if ic is None else B[..., :, ia:ia + 3] - B[..., :, ic:ic + 3]
        KR = np.stack([(K[..., 0] * R[..., 0:1, n] + K[..., 1] * R[..., 1:2, n]) + K[..., 2] * R[..., 2:3, n] for n in range(3)], axis=-1)
        Kt = np.swapaxes(K, -1, -2)
        bk = (BHt[..., :, 0:1] * Kt[..., 0:1, :] + BHt[..., :, 1:2] * Kt[..., 1:2, :]) + BHt[..., :, 2:3] * Kt[..., 2:3, :]
        kk = (KR[..., :, 0:1] * Kt[..., 0:1, :] + KR[..., :, 1:2] * Kt[..., 1:2, :]) + KR[..., :, 2:3] * Kt[..., 2:3, :]
        Pn = (B - bk) + kk
        P[:] = (Pn + np.swapaxes(Pn, -1, -2)) / 2.0
    return APPLIED, nis, y


def d_cov(key_rec, rw, s):
    """Rule 4's C from the keyframe's record and R_world [3,3]."""
    t = key_rec[..., 20:26]
    ix = [[0, 1, 2], [1, 3, 4], [2, 4, 5]]
    ct = lambda i, j: t[..., ix[i][j]]
    lead = t.shape[:-1]
    M = np.empty(lead + (3, 3)); C = np.empty(lead + (3, 3))
    for i in range(3):
        for j in range(3):
            M[..., i, j] = (rw[..., i, 0] * ct(0, j) + rw[..., i, 1] * ct(1, j)) + rw[..., i, 2] * ct(2, j)
    i2, f2 = s["infl"] * s["infl"], s["floor"] * s["floor"]
    for i in range(3):
        for j in range(i, 3):
            w = (M[..., i, 0] * rw[..., j, 0] + M[..., i, 1] * rw[..., j, 1]) + M[..., i, 2] * rw[..., j, 2]
            C[..., i, j] = i2 * w + f2 if i == j else i2 * w
            C[..., j, i] = C[..., i, j]
    return C


def clone(st):
    """Rule 7."""
    x, P = st["x"], st["P"]
    x[..., 9:12] = x[..., 0:3]
    src = [i - 9 if i >= 9 else i for i in range(N)]
    P[:] = P[..., src, :][..., :, src]
    st["istate"][1] = 1
    st["istate"][2] += 1


def step(st, s, v_uav, solved, key_rec, rw, inp=None):
    """Rules 1-8 on st = dict(x, P, istate) in place -> rec [..., 48].  v_uav [..., 3], solved, key_rec [..., 32], rw [..., 3, 3], inp
    [..., 12] or None.  Leading axes are streams that take the same path through the rules (ValueError otherwise); one stream: none."""
    x, P, ist = st["x"], st["P"], st["istate"]
    lead = x.shape[:-1]
    u = np.zeros(lead + (INPUT,)) if inp is None else np.array(np.broadcast_to(np.asarray(inp, np.float64), lead + (INPUT,)))
    v_uav = np.asarray(v_uav, np.float64); key_rec = np.asarray(key_rec, np.float64); rw = np.asarray(rw, np.float64)
    started = ist[3] == 0
    if started:
        start(st, s)
    predict(st, s, u[..., 0:3])
    out, nis, ys = [NOT] * 3, [np.zeros(lead)] * 3, [np.zeros(lead + (3,))] * 3
    if s["sigma_v"] > 0.0 and _same(np.asarray(solved) != 0) and _same(np.isfinite(v_uav).all(-1)):
        out[0], nis[0], ys[0] = update(st, 3, None, v_uav, np.diag(np.full(3, s["sigma_v"] * s["sigma_v"])), s["nis_max"])
    if _same((key_rec[..., 3] == KEY_SOLVED) & np.isfinite(key_rec[..., 10:13]).all(-1) & np.isfinite(key_rec[..., 20:26]).all(-1) &
             np.isfinite(rw).all((-1, -2))):
        C = d_cov(key_rec, rw, s)
        if ist[1] != 0:
            P[..., 9:12, 9:12] = P[..., 9:12, 9:12] + s["share"] * C
            ist[1] = 0
        out[1], nis[1], ys[1] = update(st, 0, 9, key_rec[..., 10:13], (1.0 - s["share"]) * C, s["nis_max"])
    if _same((u[..., 3] != 0.0) & np.isfinite(u[..., 4:10]).all(-1) & (u[..., 7:10] > 0.0).all(-1)):
        R = np.zeros(lead + (3, 3))
        with np.errstate(over="ignore"):                          # a sigma whose square overflows: S is not finite, refused
            for k in range(3):
                R[..., k, k] = u[..., 7 + k] * u[..., 7 + k]
        out[2], nis[2], ys[2] = update(st, 0, None, u[..., 4:7], R, s["nis_max"])
    cloned = _same(key_rec[..., 9] != 0.0)
    if cloned:
        clone(st)
    ist[0] += 1
    for k in range(3):
        if out[k] != NOT:
            ist[4 + 3 * k + out[k] - 1] += 1
    rec = np.zeros(lead + (DOUBLES,))
    rec[..., 0:12] = x
    q = 12
    for blk in (0, 3):
        for i in range(3):
            for j in range(i, 3):
                rec[..., q] = P[..., blk + i, blk + j]
                q += 1
    rec[..., 24] = (P[..., 6, 6] + P[..., 7, 7]) + P[..., 8, 8]
    for k in range(3):
        rec[..., 25 + 5 * k] = out[k]; rec[..., 26 + 5 * k] = nis[k]; rec[..., 27 + 5 * k:30 + 5 * k] = ys[k]
    rec[..., 40] = 1.0 if cloned else 0.0
    rec[..., 41] = ist[1]; rec[..., 42] = ist[0]; rec[..., 43] = ist[2]
    rec[..., 44] = (ist[4] + ist[7]) + ist[10]; rec[..., 45] = (ist[5] + ist[8]) + ist[11]; rec[..., 46] = (ist[6] + ist[9]) + ist[12]
    rec[..., 47] = 1.0 if started else 0.0
    return rec


# the record's f64 groups (a deviation is taken against the largest magnitude of its group) and the slots that must agree exactly
GROUPS = dict(p=slice(0, 3), v=slice(3, 6), b=slice(6, 9), c=slice(9, 12), P_pp=slice(12, 18), P_vv=slice(18, 24), trP_bb=slice(24, 25),
              nis=[26, 31, 36], y_v=slice(27, 30), y_D=slice(32, 35), y_fix=slice(37, 40))
EXACT = [25, 30, 35, 40, 41, 42, 43, 44, 45, 46, 47]


def key_record(D=(0.0, 0.0, 0.0), C_T=None, flag=KEY_SOLVED, reason=0):
    """A keyframe record with the fields the filter reads: flag 3, reason 9, D 10-12, C_T's upper triangle 20-25."""
    r = np.zeros(32)
    r[3] = flag; r[9] = reason; r[10:13] = D
    C = np.eye(3) * 1e-6 if C_T is None else np.asarray(C_T, np.float64)
    r[20:26] = C[np.triu_indices(3)]
    return r


def scenario(seed, steps=12000, rekey=10, sigma_D=1e-3, key_part=0.5, sigma_v=1e-3, fix_sigma=0.05, fix_every=30, walk=2e-3):
    """The experiment's truth and measurements, in units of the height d: a velocity that is a random walk (`walk` per step), a keyframe
    replaced every `rekey` steps whose D carries noise of sigma_D, of which the variance share `key_part` is drawn once per keyframe
    (the key pixels') and the rest per step, v_uav with sigma_v, a fix of fix_sigma every fix_every steps.  The keyframe's own pos
    re-anchors at every re-key (anchor = its pos there).  -> dict(p, v, D, v_uav, rekey, fix, key_pos: arrays over the steps)."""
    rng = np.random.default_rng(seed)
    v = np.zeros(3); p = np.zeros(3)
    p_key = p.copy(); e_key = rng.normal(0.0, sigma_D * np.sqrt(key_part), 3)
    anchor = np.zeros(3)
    out = dict(p=[], v=[], D=[], v_uav=[], rekey=[], fix=[], key_pos=[])
    for k in range(steps):
        p = p + v                                                # rule 2's model: the position moves with the old velocity,
        v = v + rng.normal(0.0, walk, 3)                         # which then walks; v_uav measures the new one
        D = (p - p_key) + e_key + rng.normal(0.0, sigma_D * np.sqrt(1.0 - key_part), 3)
        re = (k + 1) % rekey == 0
        out["p"].append(p.copy()); out["v"].append(v.copy()); out["D"].append(D); out["v_uav"].append(v + rng.normal(0.0, sigma_v, 3))
        out["rekey"].append(re); out["key_pos"].append(anchor + D)
        out["fix"].append(p + rng.normal(0.0, fix_sigma, 3) if (k + 1) % fix_every == 0 else np.full(3, np.nan))
        if re:
            anchor = anchor + D; p_key = p.copy(); e_key = rng.normal(0.0, sigma_D * np.sqrt(key_part), 3)
    return {k: np.array(a) for k, a in out.items()}


def run_scenario(scs, s, use_fix=True, fix_sigma=0.05, sigma_D=1e-3):
    """The restatement over the scenarios of several seeds in lockstep (they re-key and fix at the same steps) -> (p_hat [seeds, steps,
    3], P_pp [seeds, steps, 3, 3])."""
    S, n = len(scs), len(scs[0]["p"])
    st = new_state(lead=(S,))
    C_T = np.eye(3) * sigma_D * sigma_D
    rw = np.broadcast_to(np.eye(3), (S, 3, 3))
    ph, Pp = np.empty((S, n, 3)), np.empty((S, n, 3, 3))
    for k in range(n):
        inp = None
        fix = np.array([sc["fix"][k] for sc in scs])
        if use_fix and np.isfinite(fix).all():
            inp = np.zeros((S, INPUT)); inp[:, 3] = 1.0; inp[:, 4:7] = fix; inp[:, 7:10] = fix_sigma
        kr = np.array([key_record(sc["D"][k], C_T, KEY_SOLVED, 5 if sc["rekey"][k] else 0) for sc in scs])
        step(st, s, np.array([sc["v_uav"][k] for sc in scs]), 1, kr, rw, inp)
        ph[:, k] = st["x"][:, 0:3]; Pp[:, k] = st["P"][:, 0:3, 0:3]
    return ph, Pp


def experiment(seeds=range(8), steps=12000, walk=2e-3, sigma_D=1e-3, sigma_v=1e-3, fix_sigma=0.05):
    """The README's figures: rms position error of the filter, of the keyframe's own position and of the fixes alone, with and without
    fixes, and the pooled mean NEES of the position (3 is honest) with the key pixels' share modelled (share 0.5) and ignored (0)."""
    scs = [scenario(i, steps=steps, walk=walk, sigma_D=sigma_D, sigma_v=sigma_v, fix_sigma=fix_sigma) for i in seeds]
    truth = np.array([sc["p"] for sc in scs])
    rms = lambda e: float(np.sqrt((e * e).sum(-1).mean()))
    out = dict(key=rms(np.array([sc["key_pos"] for sc in scs]) - truth))
    fixes = np.array([sc["fix"] for sc in scs])
    has = np.isfinite(fixes).all(-1)
    out["fix"] = rms((fixes - truth)[has])
    for name, share, use_fix in (("filter", 0.5, True), ("filter_share0", 0.0, True), ("nofix", 0.5, False)):
        ph, Pp = run_scenario(scs, setting(sigma_v=sigma_v, q_v=walk, share=share), use_fix=use_fix, fix_sigma=fix_sigma, sigma_D=sigma_D)
        e = ph - truth
        out[name] = rms(e)
        if use_fix:
            half = steps // 2                                    # behind the transient
            w = np.linalg.solve(Pp[:, half:], e[:, half:, :, None])[..., 0]
            out["nees_" + name] = float((e[:, half:] * w).sum(-1).mean())
    return out
