"""tests/keyframe_rot_reference.py — numpy restatement of the keyframe's rotation refined from the flow (ofk.h:
ofk_set_keyframe_rotation; DESIGN.md "Keyframe rotation").

step()        rules 1', 2' and 3-5 of ofk.h in the kernel's order of operations.  The plain part of every step IS
              keyframe_reference.step: where the joint solve does not stand (or every axis is held) its state and record come back
              untouched, bit for bit.  The joint sums are added in the kernel's order (joint_reference.kernel_sum); the two 3 x 3
              eigen-decompositions come from numpy's eigh, not from a cyclic Jacobi, so delta, R^, T and the covariances are close, not
              bit-identical; flags, counts, key_xy, member and the re-key reasons are the device's bit for bit.
pair()        experiment (a): ONE keyframe/current pair of the hover geometry with a known error in R_acc; the plain key solve against
              the joint one on the same draws.
chain()       experiment (b): the hover through the full chain with default re-keying, keyframe alone against keyframe + rotation,
              with a gyro bias, white gyro noise, or the attitudes as the source.
Nothing here imports the package."""
import numpy as np

import keyframe_reference as kr
from joint_reference import EPS, kernel_sum, tri, untri

ROT_DOUBLES, ROT_STATE, MAX_ITERS = 40, 12, 8
GYRO, ATTITUDE = 0, 1
OK, NONE, SINGULAR, LARGE, HELD = 0, 1, 2, 3, 4
DEFAULTS = dict(source=GYRO, axes=(1, 1, 1), sigma_gyro=0.0, sigma_bias=1e-4, sigma_att=1e-3, iters=2, delta_max=0.1)


def setting(**kw):
    r = dict(DEFAULTS)
    r.update(kw)
    r["source"] = {"gyro": GYRO, "attitude": ATTITUDE}.get(r["source"], r["source"])
    return r


def empty(S, dtype=np.float32):
    st = kr.empty(S, dtype)
    st["rstate"] = np.zeros(ROT_STATE)
    return st


def all_held(r):
    """Every axis held by the setting alone: the plain kernel runs."""
    if not any(int(a) for a in r["axes"]):
        return True
    if r["source"] == ATTITUDE:
        return float(r["sigma_att"]) == 0.0
    return float(r["sigma_gyro"]) == 0.0 and float(r["sigma_bias"]) == 0.0


def _rows(key_xy, nxt, n, sn, nrm, R):
    """Rule 2's terms of the first n rows under the rotation R: a, b, u0, u1, sA and which rows the geometry admits."""
    d, sc, cx, cy = sn[0], sn[19], sn[20], sn[21]
    with np.errstate(all="ignore"):
        kx = (np.asarray(key_xy, np.float64)[:n, 0] - cx) * sc; ky = (np.asarray(key_xy, np.float64)[:n, 1] - cy) * sc
        px = (nxt[:n, 0].astype(np.float64) - cx) * sc; py = (nxt[:n, 1].astype(np.float64) - cy) * sc
        X = (R[0, 0] * kx + R[0, 1] * ky) + R[0, 2]; Y = (R[1, 0] * kx + R[1, 1] * ky) + R[1, 2]; Z = (R[2, 0] * kx + R[2, 1] * ky) + R[2, 2]
        den = (nrm[0] * px + nrm[1] * py) + nrm[2]
        a = X / Z; b = Y / Z
        nq = (nrm[0] * a + nrm[1] * b) + nrm[2]
        sv = nq / den
        ok = (Z >= kr.MIN_DEPTH) & (np.abs(den) >= 1e-12) & (sv > 0.0)
        u0 = sv * (px - a); u1 = sv * (py - b); sA = nq / d
    return a, b, u0, u1, sA, ok


def _terms(a, b, u0, u1, sA):
    """Per row the solve's nine sums (acc_point with q = (u, 0), sB = 1) and the eighteen of kr_point, [n, 27]."""
    with np.errstate(all="ignore"):
        q2 = np.zeros(len(a))
        k0 = b * q2 - u1; k1 = u0 - a * q2; k2 = a * u1 - b * u0
        t0 = b * k2 - k1; t1 = k0 - a * k2; t2 = a * k1 - b * k0
        pp = a * a + b * b + 1.0
        sa2 = sA * sA; sab = sA * 1.0
        cols = [sa2 * (pp - a * a), sa2 * (-a * b), sa2 * (-a), sa2 * (pp - b * b), sa2 * (-b), sa2 * (pp - 1.0), -(sab * t0), -(sab * t1), -(sab * t2)]
        n00, n01, n02, n11, n12 = pp - a * a, -a * b, -a, pp - b * b, -b
        cx = [-(a * b), 1.0 + a * a, -b]; cy = [-(1.0 + b * b), a * b, a]
        w0 = [n00 * cx[k] + n01 * cy[k] for k in range(3)]; w1 = [n01 * cx[k] + n11 * cy[k] for k in range(3)]
        w2 = [n02 * cx[k] + n12 * cy[k] for k in range(3)]
        cols += [sA * w0[k] for k in range(3)] + [sA * w1[k] for k in range(3)] + [sA * w2[k] for k in range(3)]
        cols += [cx[0] * w0[0] + cy[0] * w1[0], cx[0] * w0[1] + cy[0] * w1[1], cx[0] * w0[2] + cy[0] * w1[2],
                 cx[1] * w0[1] + cy[1] * w1[1], cx[1] * w0[2] + cy[1] * w1[2], cx[2] * w0[2] + cy[2] * w1[2]]
        q0 = n00 * u0 + n01 * u1; q1 = n01 * u0 + n11 * u1
        cols += [cx[k] * q0 + cy[k] * q1 for k in range(3)]
    return np.stack(cols, 1)


def _res2(a, b, u0, u1, sA, T):
    with np.errstate(all="ignore"):
        r0 = u0 - sA * (T[0] - T[2] * a); r1 = u1 - sA * (T[1] - T[2] * b)
        return r0 * r0 + r1 * r1


def _eig(M):
    lam, Q = np.linalg.eigh(M)
    return lam[::-1], Q[:, ::-1]


def gn_step(sums, m, lam_p, held, dl, sf2):
    """One Gauss-Newton step from the 27 sums over m rows (kr_solve) -> (ok, step, T, dict(C_delta, C_T, eig))."""
    with np.errstate(all="ignore"):
        if not np.all(np.isfinite(sums)):
            return False, None, None, None
        M = untri(sums[:6]); g = sums[6:9]; Mtd = sums[9:18].reshape(3, 3); Mdd = untri(sums[18:24]); gd = sums[24:27]
        lam, V = _eig(M)
        cut = EPS * max(3.0 * m, 3.0)
        if not (np.all(np.isfinite(lam)) and lam[2] > lam[0] * cut and lam[2] > 0.0):
            return False, None, None, None
        Mi = sum(np.outer(V[:, k], V[:, k]) / lam[k] for k in range(3))
        Y = Mi @ Mtd; t0 = Mi @ g
        S = Mdd + np.diag(lam_p) - Mtd.T @ Y
        S = (S + S.T) / 2.0
        h = (gd - lam_p * dl) - Mtd.T @ t0
        for k in range(3):
            if held[k]:
                S[k, :] = 0.0; S[:, k] = 0.0; S[k, k] = 1.0; h[k] = 0.0
        ls, U = _eig(S)
        if not (np.all(np.isfinite(ls)) and np.all(np.isfinite(h)) and ls[2] > ls[0] * cut and ls[2] > 0.0):
            return False, None, None, None
        ds = sum(U[:, k] * (U[:, k] @ h) / ls[k] for k in range(3))
        ds[np.asarray(held)] = 0.0
        T = t0 - Y @ ds
        Si = sum(np.outer(U[:, k], U[:, k]) / ls[k] for k in range(3))
        for k in range(3):
            if held[k]:
                Si[k, :] = 0.0; Si[:, k] = 0.0
    return True, ds, T, dict(C_delta=sf2 * Si, C_T=sf2 * (Mi + Y @ Si @ Y.T), eig=ls)


def prior(r, att, age, sf):
    """Rule 1': (precision per axis in the rows' units, sigma per axis, held)."""
    with np.errstate(all="ignore"):
        if att:
            var = 2.0 * (float(r["sigma_att"]) * float(r["sigma_att"]))
        else:
            var = age * (float(r["sigma_gyro"]) * float(r["sigma_gyro"])) + (age * float(r["sigma_bias"])) * (age * float(r["sigma_bias"]))
        held = [int(r["axes"][k]) == 0 or not var > 0.0 for k in range(3)]
        lam = np.array([0.0 if held[k] else (sf * sf) / var for k in range(3)])
        sig = np.array([0.0 if held[k] else np.sqrt(var) for k in range(3)])
    return lam, sig, held


def step(state, next_pts, status, n, sensors, v_uav, solved, table_step, s, r, new_count=None, max_total=None, imu=None):
    """One step of one stream with the rotation on.  keyframe_reference.step's arguments; state also carries rstate [12]; s: the
    keyframe's setting, r: the rotation's (setting()).  Returns (state, rec [32], rrec [40], count, diag)."""
    S = len(state["member"])
    sn = np.asarray(sensors, np.float64)
    rst = np.asarray(state.get("rstate", np.zeros(ROT_STATE)), np.float64)
    rrec = np.zeros(ROT_DOUBLES)
    plain_state = {k: state[k] for k in ("key_xy", "member", "state", "istate")}
    if all_held(r):
        out, rec, cnt, dg = kr.step(plain_state, next_pts, status, n, sn, v_uav, solved, table_step, s, new_count, max_total, imu)
        out["rstate"] = rst.copy(); rrec[3] = HELD
        return out, rec, rrec, cnt, dg
    ist = np.asarray(state["istate"], np.int32)
    key_step, mk = int(ist[0]), int(ist[1])
    if imu is None:
        nrm, Rw = sn[1:4], sn[7:16].reshape(3, 3)
    else:
        imu = np.asarray(imu, np.float64)
        nrm, Rw = imu[15:18], imu[6:15].reshape(3, 3)
    att = r["source"] == ATTITUDE and mk != 0 and rst[9] == 1.0 and rst[10] == float(key_step)
    if att:                                                      # R_acc from the attitudes: the plain step with omega = 0 and R_in
        K = rst[:9].reshape(3, 3)
        with np.errstate(all="ignore"):
            Racc = np.array([[(Rw[0, i] * K[0, j] + Rw[1, i] * K[1, j]) + Rw[2, i] * K[2, j] for j in range(3)] for i in range(3)])
        sn0 = sn.copy(); sn0[4:7] = 0.0
        imu0 = None
        if imu is not None:
            imu0 = imu.copy(); imu0[18:21] = 0.0
        out, rec, cnt, dg = kr.step(plain_state, next_pts, status, n, sn0, v_uav, solved, table_step, s, new_count, max_total, imu0, R_in=Racc)
    else:
        out, rec, cnt, dg = kr.step(plain_state, next_pts, status, n, sn, v_uav, solved, table_step, s, new_count, max_total, imu)
    Racc = dg["R"]
    n_ = min(max(int(n), 0), S)
    age = float((int(table_step) + 1) - key_step)
    sc = sn[19]
    sf = float(s["sigma_flow"]) * sc; gs = float(s["gate"]) * sc; g2 = gs * gs
    lam_p, sig, held = prior(r, att, age, sf)
    rrec[28:31] = sig; rrec[35] = 1.0 if att else 0.0; rrec[36] = age
    nxt = np.asarray(next_pts)
    keep = np.asarray(status).ravel()[:n_] != 0
    mem = np.asarray(state["member"]).ravel()[:n_] != 0
    jflag, jok = NONE, False
    res = None
    if rec[3] == kr.SOLVED:
        min_rows, iters = int(s["min_rows"]), int(r["iters"])

        def walk(R, inside=None):
            a, b, u0, u1, sA, ok = _rows(state["key_xy"], nxt, n_, sn, nrm, R)
            use = keep & mem & ok if inside is None else keep & mem & ok & inside
            idx = np.flatnonzero(use)
            sums = kernel_sum(_terms(a, b, u0, u1, sA)[idx], idx) if len(idx) else np.zeros(27)
            return sums, len(idx)
        a, b, u0, u1, sA, ok = _rows(state["key_xy"], nxt, n_, sn, nrm, Racc)
        idx = np.flatnonzero(keep & mem & ok)
        _, T1, _, _ = kr._solve(_terms(a, b, u0, u1, sA)[:, :9], idx, min_rows)
        rrec[32:35] = T1
        if all(held):
            jflag = HELD
        else:
            jflag = SINGULAR
            sums, m = walk(Racc)
            dl = np.zeros(3); R1 = Racc; Tj = None; cov = None
            good = True
            for it in range(1, iters + 1):
                if m < min_rows:
                    good = False; break
                okk, ds, Tj, cov = gn_step(sums, m, lam_p, held, dl, sf * sf)
                if not okk:
                    good = False; break
                dl = dl + ds
                R1 = kr.mul3(kr.rotation(dl), Racc)
                if it < iters:
                    sums, m = walk(R1)
            if good:
                rows, gated, rows2 = m, False, 0
                Rg, Tg = R1, Tj
                inside = None
                if float(s["gate"]) > 0.0:
                    ag, bg, u0g, u1g, sAg, okg = _rows(state["key_xy"], nxt, n_, sn, nrm, Rg)
                    with np.errstate(all="ignore"):
                        inside = okg & (_res2(ag, bg, u0g, u1g, sAg, Tg) <= g2)
                    d2, R2, ok2, m2 = dl.copy(), R1, True, 0
                    for it in range(1, iters + 1):
                        sums2, m2 = walk(R2, inside)
                        if it == 1:
                            rows2 = m2
                        if m2 < min_rows:
                            ok2 = False; break
                        okk, ds, T2, cov2 = gn_step(sums2, m2, lam_p, held, d2, sf * sf)
                        if not okk:
                            ok2 = False; break
                        d2 = d2 + ds
                        R2 = kr.mul3(kr.rotation(d2), Racc)
                    if ok2:
                        gated, rows, R1, dl, Tj, cov = True, m2, R2, d2, T2, cov2
                nd = float(np.sqrt((dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2]))
                if not nd <= float(r["delta_max"]):
                    jflag = LARGE if np.isfinite(nd) else SINGULAR
                    if jflag == LARGE:
                        rrec[0:3] = dl
                else:
                    a, b, u0, u1, sA, ok = _rows(state["key_xy"], nxt, n_, sn, nrm, R1)
                    use = keep & mem & ok & (inside if gated else True)
                    idx = np.flatnonzero(use)
                    ss = kernel_sum(_res2(a, b, u0, u1, sA, Tj)[idx].reshape(-1, 1), idx)[0] if len(idx) else 0.0
                    rms = float(np.sqrt(ss / len(idx)) / sc) if len(idx) else 0.0
                    jflag, jok = OK, True
                    res = dict(T=Tj, dl=dl, R=R1, cov=cov, gated=gated, rows2=rows2 if float(s["gate"]) > 0.0 else 0, rows=rows, rms=rms)
    if jok:                                                      # a displacement that is no number withdraws the joint solve: the plain step stands
        out2, rec2, cnt2, dg2, jok = _finish(state, out, rec, dg, res, Racc, nxt, keep, mem, n_, S, sn, Rw, v_uav, solved, table_step, s, new_count, max_total)
        if jok:
            out, rec, cnt, dg = out2, rec2, cnt2, dg2
        else:
            jflag = NONE; rrec[0:3] = 0.0; rrec[32:35] = 0.0
    rrec[3] = jflag
    if jok:
        rrec[0:3] = res["dl"]; rrec[13:19] = tri(res["cov"]["C_delta"]); rrec[25:28] = res["cov"]["eig"]
        rrec[31] = float(r["iters"]); rrec[37] = res["rows"]
        rrec[4:13] = res["R"].ravel()
    else:
        rrec[4:13] = Racc.ravel()
    rrec[19:25] = rec[20:26]
    rs = rst.copy()
    if dg["rekey"]:
        rs[:9] = Rw.ravel(); rs[9] = 1.0; rs[10] = float(out["istate"][0])
    out["rstate"] = rs
    dg = dict(dg); dg["Racc"] = Racc
    return out, rec, rrec, cnt, dg


def _finish(state, pout, prec, pdg, res, Racc, nxt, keep, mem, n, S, sn, Rw, v_uav, solved, table_step, s, new_count, max_total):
    """Rules 3-5 on the T and R^ of a joint solve that stands (keyframe_reference.step's, with R^ in the lever arm and the angle)."""
    st = np.asarray(state["state"], np.float64); ist = np.asarray(state["istate"], np.int32)
    key_step, mk, nkey, ndead = (int(t) for t in ist)
    anchor = st[9:12].copy(); pos = st[12:15].copy()
    off = sn[16:19]
    R, T = res["R"], res["T"]
    max_total = S if max_total is None else int(max_total)
    rec = np.zeros(kr.KEY_DOUBLES)
    with np.errstate(all="ignore"):
        cs = (((R[0, 0] + R[1, 1]) + R[2, 2]) - 1.0) / 2.0
        angle = float(np.arccos(np.fmin(1.0, np.fmax(-1.0, cs))))
        w = np.array([T[i] + (off[i] - ((R[i, 0] * off[0] + R[i, 1] * off[1]) + R[i, 2] * off[2])) for i in range(3)])
        D = np.array([(Rw[i, 0] * w[0] + Rw[i, 1] * w[1]) + Rw[i, 2] * w[2] for i in range(3)])
    flag, gated, rms = kr.SOLVED, res["gated"], res["rms"]
    jok = True
    if not np.all(np.isfinite(D)):
        return None, None, None, None, False
    pos = anchor + D
    rec[20:26] = tri(res["cov"]["C_T"])
    live = int((keep & mem).sum())
    bits = 0
    if flag != kr.SOLVED: bits |= 1
    if live < int(s["min_rows"]): bits |= 2
    if float(live) < float(s["min_share"]) * float(mk): bits |= 4
    if angle > float(s["rot_max"]): bits |= 8
    if int(s["max_age"]) > 0 and (int(table_step) + 1) - key_step > int(s["max_age"]): bits |= 16
    rekey = bits != 0
    reason = 0 if not bits else (bits & -bits).bit_length()
    out = dict(key_xy=np.array(state["key_xy"]), member=np.array(state["member"], np.uint8))
    kept = int(keep.sum())
    if rekey:
        out["key_xy"][:kept] = nxt[:n][keep]; out["member"][:kept] = 1
    else:
        out["key_xy"][:kept] = np.asarray(state["key_xy"])[:n][keep]; out["member"][:kept] = np.asarray(state["member"])[:n][keep]
    extra = 0 if new_count is None else max(0, min(int(new_count), max_total - kept, S - kept))
    out["key_xy"][kept:kept + extra] = 0; out["member"][kept:kept + extra] = 0
    if rekey:
        anchor = pos.copy()
    mk_o, ks_o, nkey_o = (kept, int(table_step) + 1, nkey + 1) if rekey else (mk, key_step, nkey)
    ndead_o = ndead + (1 if flag != kr.SOLVED else 0)
    so = np.zeros(kr.KEY_STATE)
    so[:9] = np.eye(3).ravel() if rekey else Racc.ravel()       # the source's rotation, not R^
    so[9:12] = anchor; so[12:15] = pos
    out["state"] = so; out["istate"] = np.array([ks_o, mk_o, nkey_o, ndead_o], np.int32)
    rec[0:3] = T; rec[3] = flag; rec[4] = prec[4]; rec[5] = res["rows2"]; rec[6] = rms; rec[7] = mk_o; rec[8] = ks_o; rec[9] = reason
    rec[10:13] = D; rec[13:16] = pos; rec[16:19] = anchor; rec[19] = angle; rec[26] = nkey_o; rec[27] = ndead_o; rec[28] = live
    rec[29] = 1.0 if gated else 0.0; rec[30] = bits
    dg = dict(pdg); dg.update(R=R, rekey=rekey, kept=kept, extra=extra)
    return out, rec, kept + extra, dg, jok


# ------------------------------------------------------------------------------------------------ experiment (a): one pair
def pair(err, npts=200, seed=0, noise=0.2, age=30, iters=2, sigma=None, d=10.0, gate=2.0, axes=(1, 1, 1), delta_max=0.1):
    """One keyframe (hover_pose(0)) / current frame (hover_pose(age)) pair, `noise` px on both, R_acc = exp([e]x) R_true with e drawn
    at `err` rad per axis; the prior matched (sigma = err unless given) through sigma_bias = sigma / age.  -> dict(plain, joint:
    |T - truth| / d; delta_err: |delta^ + e| (R^ = exp(delta^) exp(e) R_true); flag; in3_T, in3_d: whether T and delta^ lie inside
    3 sigma of C_T, C_delta (Mahalanobis, three degrees of freedom: 14.16); rec, rrec)."""
    rng = np.random.default_rng(1000 * seed + 17)
    S = npts
    Q = np.stack([rng.uniform(-5, 5, S), rng.uniform(-4, 4, S), np.zeros(S)], 1)
    b0, W0 = kr.hover_pose(0, d, seed)
    b1, W1 = kr.hover_pose(age, d, seed)
    key_px = kr.project(Q, b0, W0)[0] + noise * rng.standard_normal((S, 2))
    cur_px = kr.project(Q, b1, W1)[0] + noise * rng.standard_normal((S, 2))
    e = err * rng.standard_normal(3)
    Rt = W1.T @ W0
    Racc = kr.rotation(e) @ Rt
    truth = W1.T @ ((b0 + W0 @ kr.OFFSET) - (b1 + W1 @ kr.OFFSET))
    st = empty(S, np.float64)
    st["key_xy"] = key_px; st["member"][:] = 1
    st["state"][:9] = Racc.ravel(); st["istate"] = np.array([0, S, 1, 0], np.int32)
    sn = kr.sensor_row(b1, W1, np.zeros(3))
    s = kr.setting(gate=gate, rot_max=3.0)
    sg = err if sigma is None else sigma
    r = setting(sigma_gyro=0.0, sigma_bias=sg / age, iters=iters, axes=axes, delta_max=delta_max)
    status = np.ones(S, np.uint8)
    _, prec, _, _ = kr.step({k: st[k] for k in ("key_xy", "member", "state", "istate")}, cur_px, status, S, sn, np.zeros(3), False, age - 1, s)
    _, rec, rrec, _, _ = step(st, cur_px, status, S, sn, np.zeros(3), False, age - 1, s, r)
    out = dict(plain=float(np.linalg.norm(prec[0:3] - truth) / d), joint=float(np.linalg.norm(rec[0:3] - truth) / d), flag=int(rrec[3]),
               rec=rec, rrec=rrec, prec=prec, e=e, truth=truth)
    # R^ = exp(delta^) exp(e) R_true: the remaining rotation error
    left = kr.rot_log(rrec[4:13].reshape(3, 3) @ Rt.T)
    out["delta_err"] = float(np.linalg.norm(left))
    if rrec[3] == OK:
        Cd = untri(rrec[13:19]); Ct = untri(rec[20:26])
        free = [k for k in range(3) if rrec[28 + k] > 0]
        dv = left[free]
        out["in3_d"] = bool(dv @ np.linalg.solve(Cd[np.ix_(free, free)], dv) <= 14.16)
        tv = rec[0:3] - truth
        out["in3_T"] = bool(tv @ np.linalg.solve(Ct, tv) <= 14.16)
    return out


def sweep(errs=(0.0, 5e-5, 2e-4, 1e-3, 5e-3, 2e-2), npts=200, seeds=12, iters=2, **kw):
    """rms over the seeds of pair() per rotation error -> {err: dict(plain, joint, delta, in3_T, in3_d, n_ok)}."""
    out = {}
    for e in errs:
        rs = [pair(e, npts, sd, iters=iters, **kw) for sd in range(seeds)]
        okr = [x for x in rs if x["flag"] == OK]
        out[e] = dict(plain=float(np.sqrt(np.mean([x["plain"] ** 2 for x in rs]))), joint=float(np.sqrt(np.mean([x["joint"] ** 2 for x in rs]))),
                      delta=float(np.sqrt(np.mean([x["delta_err"] ** 2 for x in rs]))), n_ok=len(okr),
                      in3_T=sum(x["in3_T"] for x in okr), in3_d=sum(x["in3_d"] for x in okr))
    return out


# ------------------------------------------------------------------------------------------------ experiment (b): the hover chain
def chain(steps=200, npts=200, seed=0, noise=0.2, gyro_bias=0.0, gyro_noise=0.0, att_noise=0.0, r=None, s=None, d=10.0, report=(50, 100, 200)):
    """keyframe_reference.hover's geometry (shared observations, no deaths, no drift) through the full chain with default re-keying:
    the keyframe alone (r None) or with the rotation.  gyro_bias / gyro_noise: a constant / white error per frame in the sensors'
    omega; att_noise: a rotation error of that size per axis in the sensor rows' R_world (rows, plane normal and position's R_world
    alike see the noisy attitude only through R_world).  -> dict(key: position error / d at `report`, keyframes, flags: the
    rotation's flag per step)."""
    s = kr.setting() if s is None else s
    rng = np.random.default_rng(seed)
    S = npts
    Q = np.stack([rng.uniform(-5, 5, S), rng.uniform(-4, 4, S), np.zeros(S)], 1)
    b0, W0 = kr.hover_pose(0, d, seed)
    bp, Wp = b0, W0
    obs_prev = kr.project(Q, b0, W0)[0] + noise * rng.standard_normal((S, 2))
    key = empty(S, np.float64); one = kr.empty(S, np.float64)
    out = dict(key={}, keyframes=0, flags=[])
    dr_s = kr.setting(gate=s["gate"], min_rows=s["min_rows"], max_age=1, min_share=0.0, rot_max=3.0)
    status = np.ones(S, np.uint8)
    for k in range(1, steps + 1):
        b, W = kr.hover_pose(k, d, seed)
        om_true = kr.rot_log(W.T @ Wp)
        om = om_true + gyro_bias + gyro_noise * rng.standard_normal(3)
        obs = kr.project(Q, b, W)[0] + noise * rng.standard_normal((S, 2))
        sn = kr.sensor_row(b, W, om)
        if att_noise:
            sn[7:16] = (W @ kr.rotation(att_noise * rng.standard_normal(3))).ravel()
        one["key_xy"] = obs_prev.copy(); one["member"][:] = 1
        one["state"] = kr.empty(1)["state"]; one["istate"] = np.array([k - 1, S, 0, 0], np.int32)
        sn1 = sn.copy(); sn1[4:7] = om_true                      # the dead reckoning of the first step is not under test
        _, r1, _, _ = kr.step(one, obs, status, S, sn1, np.zeros(3), False, k - 1, dr_s)
        if r is None:
            st, rec, cnt, _ = kr.step({q: key[q] for q in ("key_xy", "member", "state", "istate")}, obs, status, S, sn, r1[10:13], r1[3] == kr.SOLVED,
                                      k - 1, s, new_count=0, max_total=S)
            st["rstate"] = key["rstate"]; key = st
        else:
            key, rec, rrec, cnt, _ = step(key, obs, status, S, sn, r1[10:13], r1[3] == kr.SOLVED, k - 1, s, r, new_count=0, max_total=S)
            out["flags"].append(int(rrec[3]))
        obs_prev = obs
        truth = -(b - b0)
        if k in report:
            out["key"][k] = float(np.linalg.norm(rec[13:16] - truth) / d)
        bp, Wp = b, W
    out["keyframes"] = int(key["istate"][2])
    return out


# ------------------------------------------------------------------------------------------------ experiment (c): rendered frames
def rendered(n_frames=12, gyro_err=(1e-3, -1e-3, 1e-3), r=None, s=None, **size):
    """keyframe_reference.rendered's sequence and tracks (the C oracle's LK with the template restatement behind it) with `gyro_err`
    added to every step's omega: the keyframe alone and the keyframe with the rotation r on the same tracks.
    -> dict(alone, rot: position error / d at the last step, flags: the rotation's per step)."""
    import track_template_reference as tr
    s = kr.setting() if s is None else s
    r = setting() if r is None else r
    seq = kr.rendered_sequence(n_frames, **size)
    cfg = tr.setting()
    h, w = seq["gray"][0].shape
    pts = seq["pts"].astype(np.float32)
    S = len(pts)
    age = np.zeros(S, np.int32)
    tstate = tr.empty_state(S, cfg.win)
    alone, rot, one = kr.empty(S), empty(S), kr.empty(S)
    dr_s = kr.setting(gate=s["gate"], min_rows=s["min_rows"], max_age=1, min_share=0.0, rot_max=3.0)
    d = float(seq["info"]["d"])
    out = dict(flags=[])
    for k in range(n_frames - 1):
        n = len(pts)
        g0, g1 = seq["gray"][k], seq["gray"][k + 1]
        nxt, st = tr.cpu_lk(g0, g1, pts)
        nxt, st = nxt.astype(np.float32), (st != 0).astype(np.uint8)
        pad = lambda a, *tail: np.concatenate([a, np.zeros((S - n,) + tail, a.dtype)])
        rec_t, L = tr.affine_fit(pts, nxt, st, n, h, w, cfg)
        nxt_s, st_s, tstate, _ = tr.template_step(g0, g1, pad(pts, 2), pad(nxt, 2), pad(st), age, n, L, tstate, cfg)
        nxt, st = nxt_s[:n], st_s[:n]
        age = np.concatenate([age[:n][st != 0] + 1, np.zeros(S - int((st != 0).sum()), np.int32)])
        sn = kr.rendered_sensors(seq, k + 1)
        sn[4:7] += np.asarray(gyro_err, np.float64)
        one["key_xy"] = pad(pts, 2); one["member"][:] = 1
        one["state"] = kr.empty(1)["state"]; one["istate"] = np.array([k, n, 0, 0], np.int32)
        _, r1, _, _ = kr.step(one, pad(nxt, 2), pad(st), n, sn, np.zeros(3), False, k, dr_s)
        alone, rec_a, _, _ = kr.step(alone, pad(nxt, 2), pad(st), n, sn, r1[10:13], r1[3] == kr.SOLVED, k, s)
        rot, rec_r, rrec, _, _ = step(rot, pad(nxt, 2), pad(st), n, sn, r1[10:13], r1[3] == kr.SOLVED, k, s, r)
        out["flags"].append(int(rrec[3]))
        pts = nxt[st != 0]
    truth = seq["truth"][n_frames - 1]
    out.update(alone=float(np.linalg.norm(rec_a[13:16] - truth) / d), rot=float(np.linalg.norm(rec_r[13:16] - truth) / d))
    return out
