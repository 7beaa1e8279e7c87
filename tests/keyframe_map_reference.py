"""tests/keyframe_map_reference.py — numpy restatement of the keyframe's map (ofk.h: ofk_set_keyframe_map; DESIGN.md "Keyframe map").

step()        rules M1-M5 of ofk.h around keyframe_reference.step(), which gives rules 1 and 2 as they stand (the rotation, the plain
              key solve, `live`); the map solve's nine sums over the live map rows in the kernel's order (joint_reference.kernel_sum);
              rules 3-5 once more on the solve that stands, in keyframe_reference's order of operations, with reason 6 beside the
              others.  key_rho, key_var, key_xy, member, mstate, the flags, the counts and the reasons are the device's bit for bit;
              T, D, pos, C_T and the spread are close, not bit-identical (another math library, eigh for the cyclic Jacobi).
experiment()  points over track_depth_reference's canopy under a camera that travels with constant (v, omega) in an exactly rigid
              world: the depth filter (track_depth_reference.step) fed the epipolar solve's v, and behind it the plane keyframe and
              the map keyframe on the same observations.
Nothing here imports the package: the tests feed it what the device downloaded."""
import numpy as np

import epi_reference as er
import keyframe_reference as kr
import track_depth_reference as td
from joint_reference import kernel_sum, tri

KEYMAP_DOUBLES = 32
USED, NONE, FEW, FELL_BACK = 0, 1, 2, 3
RE_MAP = 6
DEFAULTS = dict(min_obs=3, rel_max=0.02, min_rows=8, ready_share=0.5, weights=1)


def setting(**kw):
    m = dict(DEFAULTS)
    m.update(kw)
    return m


def empty(S, dtype=np.float32):
    st = kr.empty(S, dtype)
    st.update(key_rho=np.zeros(S), key_var=np.zeros(S), mstate=np.zeros(2, np.int32))
    return st


def clear(state, n=None):
    """k_keymap_clear on a state: the first n rows (None: all) without a key depth, captured_for = the keyframe's key_step."""
    out = dict(state)
    S = len(state["member"])
    n = S if n is None else min(max(int(n), 0), S)
    out["key_rho"] = np.array(state.get("key_rho", np.zeros(S)), np.float64); out["key_var"] = np.array(state.get("key_var", np.zeros(S)), np.float64)
    out["key_rho"][:n] = 0.0; out["key_var"][:n] = 0.0
    out["mstate"] = np.array([int(state["istate"][0]), 0], np.int32)
    return out


def mature_rows(depth, n, m):
    """Which of the first n rows of the depth state (None: none) are mature under the map setting m."""
    if depth is None:
        return np.zeros(n, bool)
    with np.errstate(all="ignore"):
        rho = np.asarray(depth["rho"], np.float64)[:n]; var = np.asarray(depth["var"], np.float64)[:n]
        nobs = np.asarray(depth["nobs"], np.int32)[:n]
        lim = float(m["rel_max"]) * rho
        return (nobs >= int(m["min_obs"])) & (rho > 0.0) & (var <= lim * lim)


def step(state, depth, next_pts, status, n, sensors, v_uav, solved, table_step, s, m, new_count=None, max_total=None, imu=None, R_in=None):
    """One step of one stream.  state: keyframe_reference's dict plus key_rho, key_var [S] and mstate [2]; depth: dict(rho, var, nobs)
    [S] as the previous depth step left it (None: no depth state); s: the keyframe's setting, m: the map's; the rest as
    keyframe_reference.step.  Returns (state, rec [32], mrec [32], count, diag)."""
    S = len(state["member"])
    n = min(max(int(n), 0), S)
    max_total = S if max_total is None else int(max_total)
    sn = np.asarray(sensors, np.float64)
    nxt = np.asarray(next_pts)
    keep = np.asarray(status).ravel()[:n] != 0
    mem = np.asarray(state["member"]).ravel()[:n] != 0
    ist = np.asarray(state["istate"], np.int32)
    key_step, mk, nkey, ndead = (int(t) for t in ist)
    cap_for, map_rows = (int(t) for t in np.asarray(state["mstate"], np.int32))
    st = np.asarray(state["state"], np.float64)
    anchor = st[9:12].copy(); pos = st[12:15].copy()
    Rw = sn[7:16].reshape(3, 3) if imu is None else np.asarray(imu, np.float64)[6:15].reshape(3, 3)
    off, sc, cx, cy = sn[16:19], sn[19], sn[20], sn[21]
    min_rows_m = int(m["min_rows"])
    # M1. capture
    krho = np.array(state["key_rho"], np.float64); kvar = np.array(state["key_var"], np.float64)
    mat = mature_rows(depth, n, m)
    capture = mk != 0 and cap_for != key_step
    captured = 0
    if capture:
        take = mem & mat
        krho[:n] = np.where(mem, np.where(take, np.asarray(depth["rho"], np.float64)[:n] if depth is not None else 0.0, 0.0), krho[:n])
        kvar[:n] = np.where(mem, np.where(take, np.asarray(depth["var"], np.float64)[:n] if depth is not None else 0.0, 0.0), kvar[:n])
        captured = int(take.sum())
        map_rows = captured
    cap_out = key_step if capture else cap_for
    # M2. the live map rows
    with np.errstate(all="ignore"):
        lm = keep & mem & (krho[:n] > 0.0)
    live_map = int(lm.sum()); ready = int((keep & mem & mat).sum())
    use_map = map_rows >= min_rows_m and live_map >= min_rows_m
    # rules 1 and 2 as they stand
    _, prec, _, dg = kr.step(state, next_pts, status, n, sensors, v_uav, solved, table_step, s, new_count, max_total, imu, R_in)
    R = dg["R"]
    live = int(prec[28])
    flag, T, rows1, rows2, rms, gated = int(prec[3]), prec[0:3].copy(), prec[4], prec[5], prec[6], prec[29] != 0.0
    CT = prec[20:26].copy()
    mrec = np.zeros(KEYMAP_DOUBLES)
    mok = False
    sf = float(s["sigma_flow"]) * sc; gs = float(s["gate"]) * sc; g2 = gs * gs; sf2 = sf * sf
    with np.errstate(all="ignore"):
        if use_map:
            # M3. the map solve
            kx = (np.asarray(state["key_xy"], np.float64)[:n, 0] - cx) * sc; ky = (np.asarray(state["key_xy"], np.float64)[:n, 1] - cy) * sc
            x = (nxt[:n, 0].astype(np.float64) - cx) * sc; y = (nxt[:n, 1].astype(np.float64) - cy) * sc
            X = (R[0, 0] * kx + R[0, 1] * ky) + R[0, 2]; Y = (R[1, 0] * kx + R[1, 1] * ky) + R[1, 2]; Z = (R[2, 0] * kx + R[2, 1] * ky) + R[2, 2]
            valid = lm & (Z >= kr.MIN_DEPTH)
            a = X / Z; b = Y / Z
            u0 = x - a; u1 = y - b; sA = krho[:n] / Z
            w = sf2 / (sf2 + ((u0 * u0 + u1 * u1) * kvar[:n]) / (krho[:n] * krho[:n])) if int(m["weights"]) else np.ones(n)
            q2 = np.zeros(n)
            k0 = y * q2 - u1; k1 = u0 - x * q2; k2 = x * u1 - y * u0
            t0 = y * k2 - k1; t1 = k0 - x * k2; t2 = x * k1 - y * k0
            pp = x * x + y * y + 1.0
            sa2 = sA * sA * w; sab = sA * 1.0 * w
            terms = np.stack([sa2 * (pp - x * x), sa2 * (-x * y), sa2 * (-x), sa2 * (pp - y * y), sa2 * (-y), sa2 * (pp - 1.0),
                              -(sab * t0), -(sab * t1), -(sab * t2)], 1)

            def res2(T):
                r0 = u0 - sA * (T[0] - T[2] * x); r1 = u1 - sA * (T[1] - T[2] * y)
                return r0 * r0 + r1 * r1
            idx = np.flatnonzero(valid)
            ok, Tm, dec, mrows1 = kr._solve(terms, idx, min_rows_m)
            mrec[3] = mrows1
            if ok:
                mok, used, mrows2, mgated = True, valid, 0, False
                T1 = Tm
                if float(s["gate"]) > 0.0:
                    inl = valid & (w * res2(T1) <= g2)
                    idx2 = np.flatnonzero(inl)
                    mrows2 = len(idx2)
                    ok2, T2, dec2, _ = kr._solve(terms, idx2, int(s["min_rows"]))
                    if ok2:
                        mgated, Tm, dec, used = True, T2, dec2, inl
                idx = np.flatnonzero(used)
                ss = kernel_sum((w * res2(Tm))[idx].reshape(-1, 1), idx)[0]
                sw = kernel_sum(w[idx].reshape(-1, 1), idx)[0]
                lam, Q = dec
                flag, T, rows1, rows2, gated = kr.SOLVED, Tm, mrows1, mrows2, mgated
                rms = float(np.sqrt(ss / len(idx)) / sc)
                CT = tri(sf2 * sum(np.outer(Q[:, k], Q[:, k]) / lam[k] for k in range(3)))
                mrec[4] = mrows2; mrec[5] = sw; mrec[6] = float(np.sqrt(ss / sw) / sc)
            if mk != 0:                                          # the plain first solve's T: the same step without a gate
                _, first, _, _ = kr.step(state, next_pts, status, n, sensors, v_uav, solved, table_step, dict(s, gate=0.0), new_count, max_total, imu, R_in)
                if first[3] == kr.SOLVED:
                    mrec[7:10] = first[0:3]
        # 3. the position, of the solve that stands
        vu = np.asarray(v_uav, np.float64)
        solved = bool(solved) and bool(np.all(np.isfinite(vu)))
        if flag == kr.SOLVED:
            wv = np.array([T[i] + (off[i] - ((R[i, 0] * off[0] + R[i, 1] * off[1]) + R[i, 2] * off[2])) for i in range(3)])
            D = np.array([(Rw[i, 0] * wv[0] + Rw[i, 1] * wv[1]) + Rw[i, 2] * wv[2] for i in range(3)])
            if np.all(np.isfinite(D)):
                pos = anchor + D
            else:
                flag, gated, rms, T = kr.UNSOLVED, False, 0.0, np.zeros(3)
                CT = np.zeros(6)
        if flag != kr.SOLVED:
            T = np.zeros(3); CT = np.zeros(6)
            if solved:
                pos = pos + vu
            D = pos - anchor
        # 4. the re-key decision, M4 beside it
        angle = prec[19]
        bits = 0
        if flag != kr.SOLVED: bits |= 1
        if live < int(s["min_rows"]): bits |= 2
        if float(live) < float(s["min_share"]) * float(mk): bits |= 4
        if angle > float(s["rot_max"]): bits |= 8
        if int(s["max_age"]) > 0 and (int(table_step) + 1) - key_step > int(s["max_age"]): bits |= 16
        if float(m["ready_share"]) > 0.0 and map_rows < min_rows_m and ready >= min_rows_m and float(ready) >= float(m["ready_share"]) * float(live):
            bits |= 32
    rekey = bits != 0
    reason = 0 if not bits else (bits & -bits).bit_length()
    # 5. compaction, M5 with it
    out = dict(key_xy=np.array(state["key_xy"]), member=np.array(state["member"], np.uint8), key_rho=np.array(state["key_rho"], np.float64),
               key_var=np.array(state["key_var"], np.float64))
    kept = int(keep.sum())
    if rekey:
        out["key_xy"][:kept] = nxt[:n][keep]; out["member"][:kept] = 1; out["key_rho"][:kept] = 0.0; out["key_var"][:kept] = 0.0
    else:
        out["key_xy"][:kept] = np.asarray(state["key_xy"])[:n][keep]; out["member"][:kept] = np.asarray(state["member"])[:n][keep]
        out["key_rho"][:kept] = krho[:n][keep]; out["key_var"][:kept] = kvar[:n][keep]
    extra = 0 if new_count is None else max(0, min(int(new_count), max_total - kept, S - kept))
    out["key_xy"][kept:kept + extra] = 0; out["member"][kept:kept + extra] = 0
    out["key_rho"][kept:kept + extra] = 0.0; out["key_var"][kept:kept + extra] = 0.0
    if rekey:
        anchor = pos.copy()
    mk_o, ks_o, nkey_o = (kept, int(table_step) + 1, nkey + 1) if rekey else (mk, key_step, nkey)
    ndead_o = ndead + (1 if flag != kr.SOLVED else 0)
    so = np.zeros(kr.KEY_STATE)
    so[:9] = np.eye(3).ravel() if rekey else R.ravel()
    so[9:12] = anchor; so[12:15] = pos
    out["state"] = so; out["istate"] = np.array([ks_o, mk_o, nkey_o, ndead_o], np.int32)
    out["mstate"] = np.array([cap_out, 0 if rekey else map_rows], np.int32)
    rec = np.zeros(kr.KEY_DOUBLES)
    rec[0:3] = T; rec[3] = flag; rec[4] = rows1; rec[5] = rows2; rec[6] = rms; rec[7] = mk_o; rec[8] = ks_o; rec[9] = reason
    rec[10:13] = D; rec[13:16] = pos; rec[16:19] = anchor; rec[19] = angle; rec[20:26] = CT; rec[26] = nkey_o; rec[27] = ndead_o; rec[28] = live
    rec[29] = 1.0 if gated else 0.0; rec[30] = bits
    mrec[0] = USED if mok else FELL_BACK if use_map else NONE if map_rows < min_rows_m else FEW
    mrec[1] = map_rows; mrec[2] = live_map; mrec[10] = captured; mrec[11] = cap_out
    diag = dict(dg, rekey=rekey, kept=kept, extra=extra, use_map=use_map, mok=mok, ready=ready)
    return out, rec, mrec, kept + extra, diag


# ------------------------------------------------------------------------------------------------ the point-level experiment
F, CX, CY = 1000.0, 640.0, 480.0
NPTS, STEPS = 300, 60


def _born(k, d, nrm, rng, kind, in_foot=0):
    """k fresh points over the frame, the first in_foot of them inside the foot, their inverse depths over the plane (nrm, d) of the
    moment with relief `kind`, and which of them are level ground inside the foot (track_depth_reference._born with the relief named)."""
    x = rng.uniform(-1.0, 1.0, (k, 2)) * [td.W2, td.H2]
    m = min(in_foot, k)
    rad, ang = 0.9 * er.FOOT * np.sqrt(rng.uniform(size=m)), rng.uniform(0, 2 * np.pi, m)
    x[:m] = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    return x, er.plane_rho(x, d, nrm) / (1.0 - er.relief(kind, x, rng)), np.hypot(x[:, 0], x[:, 1]) <= er.FOOT


def experiment(seed, kind="canopy", steps=STEPS, npts=NPTS, noise_px=0.2, v=er.V, omega=er.OM, d_wrong_from=None, d_factor=1.2, s=None, m=None, exact_v=False):
    """The experiment of DESIGN.md "Keyframe map".  npts points over ground with relief `kind`, in an exactly rigid world: every step
    P+ = R P + v with R = exp([omega]x), the ground plane with the camera.  Every frame sees every point with noise_px of independent
    error; a step's flow is the difference of two such observations, as a tracker's is.  Points that leave the frame, or carry relief
    into the foot, are replaced, track_depth_reference.FOOT_POINTS of them kept inside the foot.  Per step: the epipolar solve
    (anchor = the level foot; the range reading times d_factor from step d_wrong_from on) gives v; the plane keyframe
    (keyframe_reference.step) and the map keyframe (step) run on the same observations with the setting s (m: the map's), the map
    keyframe on the depth state as the previous step left it; then track_depth_reference.step filters the depths with that v
    (update 0 from step d_wrong_from on; exact_v: with the true v in the epipolar solve's place).  World = the camera's axes at frame 0, R_world = (R^j)^T, no lever arm; truth is the
    position in v_uav's convention, W_j T_acc with T_acc <- R T_acc + v.
    Returns dict(plane, map: |pos - truth| / d per step; flags: the map record's flag per step; keyframes: (plane's, map's); mature:
    the depth state's mature rows per step)."""
    s = kr.setting() if s is None else s
    m = setting() if m is None else m
    rng = np.random.default_rng(seed)
    v = np.asarray(v, np.float64); om = np.asarray(omega, np.float64)
    R = kr.rotation(om)
    d, nrm = er.D, er.NRM.copy()
    S = npts
    x, rho, level = _born(S, d, nrm, rng, kind, td.FOOT_POINTS)
    P = np.concatenate([x, np.ones((S, 1))], 1) / rho[:, None]
    pix = lambda x: x * F + [CX, CY]
    obs_prev = pix(x) + noise_px * rng.standard_normal((S, 2))
    plane_st, map_st, dep = kr.empty(S, np.float64), empty(S, np.float64), td.empty(S)
    ds = td.setting(sigma_flow=np.sqrt(2.0) * noise_px / F, b_min=0.5e-3)
    W, Tacc = np.eye(3), np.zeros(3)
    out = dict(plane=[], map=[], flags=[], mature=[])
    for t in range(steps):
        Pn = P @ R.T + v
        xn = Pn[:, :2] / Pn[:, 2:3]
        nrm = R @ nrm; d = d + nrm @ v                            # the plane in the new frame's axes
        gone = (np.abs(xn[:, 0]) > td.W2) | (np.abs(xn[:, 1]) > td.H2) | (~level & (np.hypot(xn[:, 0], xn[:, 1]) <= er.FOOT))
        status = (~gone).astype(np.uint8)
        obs = pix(xn) + noise_px * rng.standard_normal((S, 2))
        xs = (obs - [CX, CY]) / F; u = (obs - obs_prev) / F
        wrong = d_wrong_from is not None and t >= d_wrong_from
        d0 = d * (d_factor if wrong else 1.0)
        ep = er.epi_solve(xs[~gone], u[~gone], d0, nrm, om, anchor=er.FOOT, fast=True)
        ok = ep["flag"] == 0
        if exact_v:                                              # the depths fed the true v: what is left is the filter's own
            ep, ok = dict(v=v.copy()), True
        W = W @ R.T; Tacc = R @ Tacc + v
        truth = W @ Tacc
        sn = np.zeros(28)
        sn[0] = d0; sn[1:4] = nrm; sn[4:7] = om; sn[7:16] = W.ravel(); sn[19] = 1.0 / F; sn[20] = CX; sn[21] = CY
        born = int(gone.sum())
        plane_st, prec, _, _ = kr.step(plane_st, obs, status, S, sn, W @ ep["v"], ok, t, s, new_count=born, max_total=S)
        map_st, krec, mrec, _, _ = step(map_st, dep, obs, status, S, sn, W @ ep["v"], ok, t, s, m, new_count=born, max_total=S)
        out["mature"].append(int(mature_rows(dep, S, m).sum()))
        dep, _, _, _ = td.step(dep, xs, u, status, S, om, ep["v"], ok, dict(ds, update=0) if wrong else ds, new_count=born, max_total=S)
        out["plane"].append(float(np.linalg.norm(prec[13:16] - truth) / er.D)); out["map"].append(float(np.linalg.norm(krec[13:16] - truth) / er.D))
        out["flags"].append(int(mrec[0]))
        kept = S - born
        stay = xn[~gone]
        xb, rb, lb = _born(born, d, nrm, rng, kind, max(0, td.FOOT_POINTS - int((np.hypot(stay[:, 0], stay[:, 1]) <= er.FOOT).sum())))
        P = np.concatenate([Pn[~gone], np.concatenate([xb, np.ones((born, 1))], 1) / rb[:, None]])
        level = np.concatenate([level[~gone], lb])
        obs_prev = np.concatenate([obs[~gone], pix(xb) + noise_px * rng.standard_normal((born, 2))])
    out["keyframes"] = (int(plane_st["istate"][2]), int(map_st["istate"][2]))
    return out
