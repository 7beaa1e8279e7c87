"""numpy restatement of the track templates (include/ofk.h: ofk_set_track_template), rules 1-6 for one stream: the image sums are
integers in int64, the f32 and f64 steps are taken in the order the header states, so rules 2-6 agree with the device bit for bit; rule
1 goes through numpy's eigh instead of the kernel's Jacobi and agrees to rounding (1e-10 relative).

Also the experiment behind the feature: the C oracle's LK chain over a rendered sequence with and without the restatement behind every
LK step (run_sequence), measured against the homography of the rendered plane."""
from types import SimpleNamespace

import numpy as np

F = np.float32
EPS = 2.220446049250313e-16
DOUBLES = 32
NOT_TRACKED, PASS, FAIL, ABANDONED, OUTSIDE, FLAT, NO_TEMPLATE, CAPTURED = 0, 1, 2, 3, 4, 5, 6, 16
KEEP, DROP = 0, 1


def setting(win=15, ncc_min=0.8, anchor_iters=3, anchor_max=2.0, outside=KEEP, fit_min=6, fit_gate=2.0, scale_max=1.5):
    return SimpleNamespace(win=win, ncc_min=ncc_min, anchor_iters=anchor_iters, anchor_max=anchor_max, outside=outside, fit_min=fit_min,
                           fit_gate=fit_gate, scale_max=scale_max)


def tpl_stride(win):
    return ((win + 2) ** 2 + 3) // 4 * 4


def empty_state(S, win):
    A = np.zeros((S, 4), F)
    return dict(tmpl=np.zeros((S, tpl_stride(win)), np.uint8), A=A, ncc=np.zeros(S, F), flag=np.zeros(S, np.uint8), tstate=np.zeros(S, np.uint8))


# ---------------------------------------------------------------------------------------------------------------- the sampler
def sample(img, px, py, A, ox, oy):
    """S(img, p, A, o) for integer offset arrays ox, oy -> (values int64 at scale 1024, outside bool)."""
    h, w = img.shape
    with np.errstate(all="ignore"):
        fx, fy = ox.astype(F), oy.astype(F)
        sx = (F(A[0]) * fx + F(A[1]) * fy) + F(px)
        sy = (F(A[2]) * fx + F(A[3]) * fy) + F(py)
        ixf, iyf = np.floor(sx), np.floor(sy)
        ok = (ixf >= F(0)) & (iyf >= F(0)) & (ixf + F(1) <= F(w - 1)) & (iyf + F(1) <= F(h - 1))
        ix = np.where(ok, ixf, 0).astype(np.int64); iy = np.where(ok, iyf, 0).astype(np.int64)
        qx = np.where(ok, np.rint((sx - ixf) * F(32)), 0).astype(np.int64); qy = np.where(ok, np.rint((sy - iyf) * F(32)), 0).astype(np.int64)
    I = img.astype(np.int64)
    v = (I[iy, ix] * (32 - qx) * (32 - qy) + I[iy, ix + 1] * qx * (32 - qy)) + (I[iy + 1, ix] * (32 - qx) * qy + I[iy + 1, ix + 1] * qx * qy)
    return v, ~ok


def offsets(e, half):
    """The e x e grid of offsets -half..half, row-major."""
    k = np.arange(e * e)
    return k % e - half, k // e - half


def capture(img, px, py, win):
    """Rule 2 -> the (win+2)^2 template bytes, or None where a sample is outside."""
    ox, oy = offsets(win + 2, (win - 1) // 2 + 1)
    v, out = sample(img, px, py, (1.0, 0.0, 0.0, 1.0), ox, oy)
    return None if out.any() else ((v + 512) >> 10).astype(np.uint8)


def template_terms(tmpl, win):
    """T and g over the inner window, int64, and the template's own sums."""
    e = win + 2
    T2 = tmpl[:e * e].astype(np.int64).reshape(e, e)
    T = T2[1:-1, 1:-1].ravel()
    gx = (T2[1:-1, 2:] - T2[1:-1, :-2]).ravel(); gy = (T2[2:, 1:-1] - T2[:-2, 1:-1]).ravel()
    return T, gx, gy


def window_sums(img, px, py, A, T, gx, gy, ox, oy):
    J, out = sample(img, px, py, A, ox, oy)
    if out.any():
        return None
    D = J - 1024 * T
    return dict(J=int(J.sum()), JJ=int((J * J).sum()), TJ=int((T * J).sum()), gxD=int((gx * D).sum()), gyD=int((gy * D).sum()))


def score_row(img, p0, An, tmpl, cfg):
    """Rules 3-5 for one row with a template -> (p [2] f32, ncc f32, flag, drop)."""
    win = cfg.win; N = win * win
    T, gx, gy = template_terms(tmpl, win)
    ox, oy = offsets(win, (win - 1) // 2)
    sT, sTT = int(T.sum()), int((T * T).sum())
    sgx, sgy, sxx, sxy, syy = int(gx.sum()), int(gy.sum()), int((gx * gx).sum()), int((gx * gy).sum()), int((gy * gy).sum())
    vT = N * sTT - sT * sT
    G00, G01, G11 = float(N * sxx - sgx * sgx), float(N * sxy - sgx * sgy), float(N * syy - sgy * sgy)
    det = G00 * G11 - G01 * G01
    p0x, p0y = F(p0[0]), F(p0[1])
    px, py = p0x, p0y
    s = window_sums(img, px, py, An, T, gx, gy, ox, oy)
    if s is None:
        return (p0x, p0y), F(0), OUTSIDE, cfg.outside == DROP
    if vT <= 0 or N * s["JJ"] - s["J"] * s["J"] <= 0:
        return (p0x, p0y), F(0), FLAT, False
    s0, abandoned = s, False
    a = [float(F(x)) for x in An]
    if det > 0.0:
        for _ in range(cfg.anchor_iters):
            sD = s["J"] - 1024 * sT
            bx, by = float(N * s["gxD"] - sgx * sD), float(N * s["gyD"] - sgy * sD)
            with np.errstate(all="ignore"):
                dx = np.float64(G11 * bx - G01 * by) / det / 512.0; dy = np.float64(G00 * by - G01 * bx) / det / 512.0
                sx = a[0] * dx + a[1] * dy; sy = a[2] * dx + a[3] * dy
                qx = F(np.float64(px) - sx); qy = F(np.float64(py) - sy)
                am = F(cfg.anchor_max)
                if not (np.isfinite(sx) and np.isfinite(sy)) or not (np.abs(qx - p0x) <= am and np.abs(qy - p0y) <= am):
                    abandoned = True
                    break
            sn = window_sums(img, qx, qy, An, T, gx, gy, ox, oy)
            if sn is None:
                abandoned = True
                break
            px, py, s = qx, qy, sn
            if sx * sx + sy * sy < 1e-4:
                break
    if abandoned:
        px, py, s = p0x, p0y, s0
    vJ, cTJ = N * s["JJ"] - s["J"] * s["J"], N * s["TJ"] - sT * s["J"]
    if vJ <= 0:
        return (p0x, p0y), F(0), FLAT, False
    rho = float(cTJ) / np.sqrt(float(vT) * float(vJ))
    if rho < cfg.ncc_min:
        return (p0x, p0y), F(rho), FAIL, True
    return (px, py), F(rho), ABANDONED if abandoned else PASS, False


def mul_LA(L, a):
    """A' = L A, each entry L_r0 a_0c + L_r1 a_1c in f32."""
    L = [F(x) for x in L]; a = [F(x) for x in a]
    with np.errstate(all="ignore"):
        return np.array([L[0] * a[0] + L[1] * a[2], L[0] * a[1] + L[1] * a[3], L[2] * a[0] + L[3] * a[2], L[2] * a[1] + L[3] * a[3]], F)


# ---------------------------------------------------------------------------------------------------------------- rule 1
def _fit(x, y):
    """The least squares of both coordinates from the normal equations -> (M [4], t [2]) or None (rank < 3, not finite)."""
    z = np.column_stack([x, np.ones(len(x))])
    with np.errstate(all="ignore"):
        Nm = z.T @ z; g = z.T @ y
    if not (np.isfinite(Nm).all() and np.isfinite(g).all()):
        return None
    lam, V = np.linalg.eigh(Nm)
    tol = lam.max() * EPS * max(len(x), 3.0)
    if not (lam > tol).all() or not (lam > 0).all():
        return None
    u = V @ ((V.T @ g) / lam[:, None])                           # [3, 2]
    return np.array([u[0, 0], u[1, 0], u[0, 1], u[1, 1]]), np.array([u[2, 0], u[2, 1]])


def affine_fit(prev_pts, next_pts, status, n, h, w, cfg):
    """Rule 1 for one stream -> (rec [32] with slots 0-9 filled, L [4] f32)."""
    rec = np.zeros(DOUBLES); rec[0] = rec[3] = 1.0; rec[6] = 1.0
    k = np.flatnonzero(np.asarray(status[:n]) != 0)
    c = np.array([w * 0.5, h * 0.5])
    x = np.asarray(prev_pts, F)[k].astype(np.float64) - c; y = np.asarray(next_pts, F)[k].astype(np.float64) - c
    rec[7] = len(k)
    first = _fit(x, y) if len(k) >= cfg.fit_min else None
    if first is not None:
        M, t = first
        res = lambda M, t: (((M[0] * x[:, 0] + M[1] * x[:, 1]) + t[0]) - y[:, 0]) ** 2 + (((M[2] * x[:, 0] + M[3] * x[:, 1]) + t[1]) - y[:, 1]) ** 2
        rr = res(M, t)
        if cfg.fit_gate > 0.0:
            inl = rr <= cfg.fit_gate * cfg.fit_gate
            rec[8] = inl.sum()
            sec = _fit(x[inl], y[inl]) if inl.sum() >= cfg.fit_min else None
            if sec is not None:
                M, t = sec
                rr = res(M, t)[inl]
        rec[0:4], rec[4:6], rec[6] = M, t, 0.0
        rec[9] = np.sqrt(rr.sum() / len(rr)) if len(rr) else 0.0
    return rec, rec[0:4].astype(F)


# ---------------------------------------------------------------------------------------------------------------- rules 2-6
def template_step(prev_img, next_img, prev_pts, next_pts, status, age, n, L, state, cfg, new_count=None, max_total=None):
    """ofk_track_template_step for one stream: arrays over S rows -> (next_pts, status: rows as tracked; state: compacted; rec)."""
    S = len(status)
    max_total = S if max_total is None else max_total
    nxt = np.array(next_pts, F); st = np.array(status, np.uint8)
    tm, A, tstate = state["tmpl"].copy(), state["A"].copy(), state["tstate"].copy()
    A_new = np.zeros((S, 4), F); ncc_new = np.zeros(S, F); flag_new = np.zeros(S, np.uint8); move = np.zeros(S, F)
    e2 = (cfg.win + 2) ** 2
    for r in range(n):
        has, captured = tstate[r] != 0 and age[r] != 0, False
        a = A[r]
        if not has:
            t = capture(prev_img, prev_pts[r][0], prev_pts[r][1], cfg.win)
            captured = has = t is not None
            tstate[r] = 1 if has else 0
            a = np.array([1, 0, 0, 1], F)
            if has:
                tm[r, :e2] = t; A[r] = a
        An = mul_LA(L, a)
        p, ncc, flag, drop = (nxt[r, 0], nxt[r, 1]), F(0), NOT_TRACKED, False
        if st[r] != 0:
            if not has:
                flag = NO_TEMPLATE
            else:
                p, ncc, flag, drop = score_row(next_img, nxt[r], An, tm[r], cfg)
        A_new[r], ncc_new[r], flag_new[r] = An, ncc, flag | (CAPTURED if captured else 0)
        move[r] = max(abs(F(p[0]) - nxt[r, 0]), abs(F(p[1]) - nxt[r, 1]))
        if drop:
            st[r] = 0
        else:
            nxt[r] = p
    # rule 6
    # the templates move into a second buffer that started as the input's copy
    out = dict(tmpl=state["tmpl"].copy(), A=A.copy(), ncc=state["ncc"].copy(), flag=state["flag"].copy(), tstate=tstate.copy())
    rec = np.zeros(DOUBLES)
    verdict = flag_new[:n] & 15
    keep = np.flatnonzero(st[:n] != 0)
    s2, s2i = F(cfg.scale_max * cfg.scale_max), F(1.0 / (cfg.scale_max * cfg.scale_max)) if cfg.scale_max > 0 else F(0)
    refreshed = 0
    for q, r in enumerate(keep):
        ts = tstate[r]
        with np.errstate(all="ignore"):
            det = A_new[r, 0] * A_new[r, 3] - A_new[r, 1] * A_new[r, 2]
        if ts != 0 and cfg.scale_max > 0 and not (det <= s2 and det >= s2i):
            ts = 0; refreshed += 1
        out["tmpl"][q] = tm[r]; out["A"][q] = A_new[r]; out["ncc"][q] = ncc_new[r]; out["flag"][q] = flag_new[r]; out["tstate"][q] = ts
    kept = len(keep)
    extra = max(0, min(new_count, max_total - kept, S - kept)) if new_count is not None else 0
    for q in range(kept, kept + extra):
        out["A"][q] = (1, 0, 0, 1); out["ncc"][q] = 0; out["flag"][q] = 0; out["tstate"][q] = 0
    moved = (verdict == PASS) & (move[:n] > 0)
    rec[10] = np.isin(verdict, (PASS, FAIL, ABANDONED)).sum()
    rec[11] = ((verdict == FAIL) | ((verdict == OUTSIDE) & (cfg.outside == DROP))).sum()
    rec[12] = moved.sum(); rec[13] = (verdict == ABANDONED).sum(); rec[14] = (verdict == OUTSIDE).sum(); rec[15] = (verdict == FLAT).sum()
    rec[16] = ((flag_new[:n] & CAPTURED) != 0).sum(); rec[17] = (verdict == NO_TEMPLATE).sum(); rec[18] = refreshed
    rec[19] = move[:n][moved].max() if moved.any() else 0.0
    return nxt, st, out, rec


# ---------------------------------------------------------------------------------------------------------------- the experiment
SEQUENCES = {
    "yaw": dict(v=(.003, -.002, 0.0), omega=(0.0, 0.0, .02)),
    "climb": dict(v=(.002, .001, .012), omega=(.001, -.001, .005)),
    "fast": dict(v=(.02, -.015, .004), omega=(.004, -.003, .03)),
}
H_SEQ, W_SEQ, SEED_SEQ, CORNERS = 480, 640, 5, 300
_seqs = {}


def sequence(name, n_frames=30):
    """The gray frames of a sequence, its per-frame homography and the 300 corners of frame 0 (cached per process)."""
    key = (name, n_frames)
    if key not in _seqs:
        import os
        import sys
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        if root not in sys.path:
            sys.path.insert(0, root)
        from __graft_entry__ import load_package
        load_package()
        from of_amd import synth
        from oracle import image_oracle as io
        frames, info = synth.render_sequence(H_SEQ, W_SEQ, SEED_SEQ, n_frames, **SEQUENCES[name])
        gray = [io.gray_bgr8(f) for f in frames]
        pts = io.good_features(gray[0], CORNERS, 0.01, 10, 3).reshape(-1, 2)
        _seqs[key] = dict(gray=gray, bgr=frames, H=info["H"], pts=pts, info=info)
    return _seqs[key]


def project(H, pts):
    p = np.concatenate([np.asarray(pts, np.float64).reshape(-1, 2), np.ones((len(pts), 1))], 1) @ H.T
    return p[:, :2] / p[:, 2:3]


def cpu_lk(g0, g1, pts):
    from oracle import image_oracle as io
    n, s, _ = io.lk_pyr(g0, g1, pts, win=15, max_level=3)
    return n.reshape(-1, 2), s.ravel()


def run_sequence(name, cfg=None, n_frames=30, lk=cpu_lk):
    """The tracks of frame 0 through n_frames - 1 steps without re-detection; cfg None: LK and its status alone, else the restatement
    behind every LK step.  -> per step dict(birth [m,2] the birth positions of the live tracks, pts [m,2] where they are, err [m] the
    distance from H^k(birth), inside [m] whether the truth's window lies in the frame, ncc [m], flag [m])."""
    seq = sequence(name, n_frames)
    pts, birth = seq["pts"].astype(F), seq["pts"].astype(np.float64)
    S = len(pts)
    age = np.zeros(S, np.int32)
    state = empty_state(S, cfg.win) if cfg is not None else None
    Hk, out = np.eye(3), []
    half = 8 if cfg is None else (cfg.win - 1) // 2 + 1
    for k in range(n_frames - 1):
        n = len(pts)
        g0, g1 = seq["gray"][k], seq["gray"][k + 1]
        nxt, st = (np.zeros((0, 2), F), np.zeros(0, np.uint8)) if n == 0 else lk(g0, g1, pts)
        nxt, st = nxt.astype(F), (st != 0).astype(np.uint8)
        ncc, flag = np.zeros(n, F), np.zeros(n, np.uint8)
        if cfg is not None and n:
            pad = lambda a, *tail: np.concatenate([a, np.zeros((S - n,) + tail, a.dtype)])
            rec, L = affine_fit(pts, nxt, st, n, H_SEQ, W_SEQ, cfg)
            nxt_s, st_s, state, _ = template_step(g0, g1, pad(pts, 2), pad(nxt, 2), pad(st), age, n, L, state, cfg)
            nxt, st = nxt_s[:n], st_s[:n]
            kept = int((st != 0).sum())
            ncc, flag = state["ncc"][:kept], state["flag"][:kept]
            age = np.concatenate([age[:n][st != 0] + 1, np.zeros(S - kept, np.int32)])
        Hk = seq["H"] @ Hk
        keep = st != 0
        pts, birth = nxt[keep], birth[keep]
        truth = project(Hk, birth)
        inside = (truth[:, 0] >= half + 1) & (truth[:, 0] <= W_SEQ - 2 - half) & (truth[:, 1] >= half + 1) & (truth[:, 1] <= H_SEQ - 2 - half)
        out.append(dict(birth=birth.copy(), pts=pts.copy(), err=np.hypot(*(pts.astype(np.float64) - truth).T), inside=inside, ncc=np.array(ncc),
                        flag=np.array(flag)))
    return out


def summary(step):
    """(median, p90 drift in px, tracks within 0.5 px, tracks alive) of one step of run_sequence."""
    e = step["err"]
    if not len(e):
        return float("nan"), float("nan"), 0, 0
    return float(np.median(e)), float(np.percentile(e, 90)), int((e <= 0.5).sum()), len(e)
