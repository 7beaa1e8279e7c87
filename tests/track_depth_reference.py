"""tests/track_depth_reference.py — numpy restatement of the depth per track (ofk.h: ofk_set_track_depth; DESIGN.md "Depth per track").

step()        rules 1-4 of ofk.h in the kernel's order of operations: the map solve's nine sums over the mature rows in the kernel's
              order (joint_reference.kernel_sum), measurement, prediction and compaction elementwise in float64 - every operation is
              one of + - * / and a square root that only feeds comparisons, so rho, var, nobs and the counts are the device's bit for
              bit.  The 3 x 3 eigen-decomposition comes from numpy's eigh, not from a cyclic Jacobi: v_map and C_map are close, not
              bit-identical.
experiment()  points over relief, 40 steps of constant (v, omega): positions advanced by the exact flow, depths by Z+ = Z g, the
              per-step v from epi_reference.epi_solve; what the filter gains over the single frame, and v_map against the other solves.
Nothing here imports the package: the tests feed it what the device downloaded."""
import numpy as np

import epi_reference as er
from joint_reference import EPS, kernel_sum, plain_solve, NODE, tri, untri

TD_DOUBLES = 32
DEFAULTS = dict(sigma_flow=0.2, b_min=0.5, gate=3.0, q=0.0, min_obs=3, rel_max=0.25, min_rows=8, update=1)


def setting(**kw):
    s = dict(DEFAULTS)
    s.update(kw)
    return s


def empty(S):
    return dict(rho=np.zeros(S), var=np.zeros(S), nobs=np.zeros(S, np.int32))


def step(state, x, u, status, n, omega, v, solved, s, new_count=None, max_total=None, scale=1.0):
    """One step of one stream.  state: dict(rho, var, nobs) over the stride S; x, u [S,2] the solve's points; status [S]; n the rows in
    use; omega, v [3]; s: a setting (sigma_flow and b_min are multiplied by `scale`, the stream's scaling in the resident paths).
    Returns (state, rec [32], count, diag): the new state over S (rows behind the count as they were), diag the per-row z, R and
    keep flags of the rows 0..n-1."""
    S = len(state["rho"])
    n = min(max(int(n), 0), S)
    max_total = S if max_total is None else int(max_total)
    x = np.asarray(x, np.float64).reshape(-1, 2)[:n]; u = np.asarray(u, np.float64).reshape(-1, 2)[:n]
    keep = np.asarray(status).ravel()[:n] != 0
    rho = np.asarray(state["rho"], np.float64)[:n].copy(); var = np.asarray(state["var"], np.float64)[:n].copy()
    nobs = np.asarray(state["nobs"], np.int32)[:n].copy()
    om = [float(t) for t in omega]; vv = [float(t) for t in v]
    sf = float(s["sigma_flow"]) * scale; bmin = float(s["b_min"]) * scale
    sf2 = sf * sf; g2 = float(s["gate"]) * float(s["gate"]); gs = g2 * sf2
    gate_on = float(s["gate"]) > 0.0
    q = float(s["q"])
    meas = bool(solved) and all(np.isfinite(vv))
    rec = np.zeros(TD_DOUBLES)
    with np.errstate(all="ignore"):
        xs, ys = x[:, 0], x[:, 1]
        c0 = ys * om[2] - om[1]; c1 = om[0] - xs * om[2]; c2 = xs * om[1] - ys * om[0]       # [p]x omega
        q0 = u[:, 0] + c0; q1 = u[:, 1] + c1; q2 = c2
        # 1. the map solve from the prior state
        lim = float(s["rel_max"]) * rho
        mature = keep & (nobs >= int(s["min_obs"])) & (rho > 0.0) & (var <= lim * lim)
        idx = np.flatnonzero(mature)
        m = len(idx)
        flag = 1.0
        if m:
            X, Y, r = xs[idx], ys[idx], rho[idx]
            k0 = Y * q2[idx] - q1[idx]; k1 = q0[idx] - X * q2[idx]; k2 = X * q1[idx] - Y * q0[idx]      # X q
            t0 = Y * k2 - k1; t1 = k0 - X * k2; t2 = X * k1 - Y * k0                                # X X q
            pp = X * X + Y * Y + 1.0
            sa2 = r * r; sab = r * 1.0
            terms = np.stack([sa2 * (pp - X * X), sa2 * (-X * Y), sa2 * (-X), sa2 * (pp - Y * Y), sa2 * (-Y), sa2 * (pp - 1.0),
                              -(sab * t0), -(sab * t1), -(sab * t2)], 1)
            sums = kernel_sum(terms, idx)
            if m >= int(s["min_rows"]) and np.all(np.isfinite(sums)):
                M = untri(sums[:6]); g = sums[6:9]
                lam, Q = np.linalg.eigh(M)
                lam = lam[::-1]; Q = Q[:, ::-1]
                tol = lam[0] * EPS * max(3.0 * m, 3.0)
                if np.all(np.isfinite(lam)) and all(l > tol and l > 0 for l in lam):
                    vm = sum(Q[:, k] * (Q[:, k] @ g) / lam[k] for k in range(3))
                    C = sf2 * sum(np.outer(Q[:, k], Q[:, k]) / lam[k] for k in range(3))
                    rec[0:3] = vm; rec[10:16] = tri(C); flag = 0.0
        rec[3] = flag; rec[4] = m
        # 2. measurement
        a0 = q0 - q2 * xs; a1 = q1 - q2 * ys; b0 = vv[0] - vv[2] * xs; b1 = vv[1] - vv[2] * ys
        bb = b0 * b0 + b1 * b1; ab = a0 * b0 + a1 * b1; nb = np.sqrt(bb)
        cr = a0 * b1 - a1 * b0; kap = ab / bb; rr = cr / nb
        on = keep & meas
        skb = on & (nb < bmin)
        skr = on & ~skb & gate_on & (rr * rr > gs)
        skb = skb | (on & ~skb & ~skr & ~np.isfinite(kap))
        ok = on & ~skb & ~skr
        R = sf2 / bb
        ini = ok & (nobs == 0) & (kap > 0.0)
        cand = ok & (nobs != 0) & bool(s["update"])
        nu = kap - rho; Sv = var + R
        sknu = cand & gate_on & (nu * nu > g2 * Sv)
        upd = cand & ~sknu
        K = var / Sv
        rho1 = np.where(ini, kap, np.where(upd, rho + K * nu, rho))
        var1 = np.where(ini, R, np.where(upd, var * R / Sv, var))
        nobs1 = np.where(ini, 1, np.where(upd, nobs + 1, nobs)).astype(np.int32)
        # 3. prediction
        has = keep & (nobs1 >= 1)
        w = om[0] * ys - om[1] * xs
        g = (1.0 + rho1 * vv[2]) + w
        good = np.isfinite(g) & (g >= 0.1)
        J = (1.0 + w) / (g * g)
        if solved:
            pred = has & good; rst = has & ~good
            rho2 = np.where(pred, rho1 / g, np.where(rst, 0.0, rho1))
            var2 = np.where(pred, var1 * J * J + q, np.where(rst, 0.0, var1))
            nobs2 = np.where(rst, 0, nobs1).astype(np.int32)
        else:
            rst = np.zeros(n, bool)
            rho2, var2, nobs2 = rho1, np.where(has, var1 + q, var1), nobs1
    rec[5] = upd.sum(); rec[6] = ini.sum(); rec[7] = skb.sum(); rec[8] = skr.sum(); rec[9] = sknu.sum()
    rec[16:19] = vv; rec[19] = 1.0 if solved else 0.0; rec[20] = rst.sum()
    # 4. compaction
    out = {k: np.array(state[k]) for k in ("rho", "var", "nobs")}
    kept = int(keep.sum())
    out["rho"][:kept] = rho2[keep]; out["var"][:kept] = var2[keep]; out["nobs"][:kept] = nobs2[keep]
    extra = 0 if new_count is None else max(0, min(int(new_count), max_total - kept, S - kept))
    out["rho"][kept:kept + extra] = 0.0; out["var"][kept:kept + extra] = 0.0; out["nobs"][kept:kept + extra] = 0
    diag = dict(z=kap, R=R, keep=keep, used=ini | upd, mature=mature)
    return out, rec, kept + extra, diag


def record_scale(rec):
    """Per-slot scales of a depth record for the 1e-9 comparison: v_map relative to its largest component, C_map to its largest entry."""
    rec = np.asarray(rec, np.float64)
    sc = np.ones(TD_DOUBLES)
    for lo, hi in ((0, 3), (10, 16)):
        sc[lo:hi] = max(np.abs(rec[lo:hi]).max(), 1e-300)
    return sc


# ---- the point-level experiment
W2, H2 = 0.64, 0.48                                             # half a 1280 x 960 frame at f = 1000
NPTS, STEPS = 300, 40


FOOT_POINTS = 10                                                # level points kept inside the foot: the epipolar solve's anchor set


def _born(k, d, nrm, rng, in_foot=0):
    """k fresh points over the frame, the first in_foot of them inside the foot, and their inverse depths on the canopy over the
    plane (nrm, d) of the moment."""
    x = rng.uniform(-1.0, 1.0, (k, 2)) * [W2, H2]
    m = min(in_foot, k)
    rad, ang = 0.9 * er.FOOT * np.sqrt(rng.uniform(size=m)), rng.uniform(0, 2 * np.pi, m)
    x[:m] = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    return x, er.plane_rho(x, d, nrm) / (1.0 - er.relief("canopy", x, rng)), np.hypot(x[:, 0], x[:, 1]) <= er.FOOT


def experiment(seed, s=None, steps=STEPS, npts=NPTS, noise=er.SIGMA_FLOW, v=er.V, omega=er.OM, d_wrong_from=None, d_factor=1.2,
               freeze_from=None):
    """The experiment of DESIGN.md "Depth per track".  npts points, each step: the flow of (v, omega) at the points' true inverse
    depths plus `noise`; the epipolar solve (anchor = the level foot, the range reading d0 - times d_factor from step d_wrong_from on)
    gives the step's v (a step where it declines counts as not solved); step() filters with it (update 0 from step freeze_from on); positions
    move on by the exact flow, depths by Z+ = Z g, the ground plane with the camera; points that leave the frame, or carry relief into
    the foot, are replaced, FOOT_POINTS of them kept inside the foot.  Returns one dict per step: v_epi, v_plain, v_map, flag, mature, and per row of the step rho_true (at the
    measurement), z, rho_prior, var_prior, nobs_prior, and after the step rho_post / var_post / nobs_post against rho_next."""
    s = setting(sigma_flow=noise, b_min=0.5e-3) if s is None else s
    rng = np.random.default_rng(seed)
    v = np.asarray(v, np.float64); om = np.asarray(omega, np.float64)
    d, nrm = er.D, er.NRM.copy()
    x, rho, level = _born(npts, d, nrm, rng, FOOT_POINTS)
    st = empty(npts)
    A = np.eye(3) + np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
    Ai = np.linalg.inv(A)
    out = []
    for t in range(steps):
        u_true = er.flow(x, v, om, rho)
        u = u_true + rng.normal(0, noise, u_true.shape)
        d0 = d * (d_factor if d_wrong_from is not None and t >= d_wrong_from else 1.0)
        ep = er.epi_solve(x, u, d0, nrm, om, anchor=er.FOOT, fast=True)
        v_plain = plain_solve(NODE, x, u, d0, nrm, om)[0]
        v_used = ep["v"]
        g = 1.0 + rho * v[2] + (om[0] * x[:, 1] - om[1] * x[:, 0])
        x_next = x + u_true; rho_next = rho / g
        gone = (np.abs(x_next[:, 0]) > W2) | (np.abs(x_next[:, 1]) > H2) | (~level & (np.hypot(x_next[:, 0], x_next[:, 1]) <= er.FOOT))
        status = (~gone).astype(np.uint8)
        ss = dict(s, update=0) if freeze_from is not None and t >= freeze_from else s
        prior = {k: a.copy() for k, a in st.items()}
        st, rec, count, diag = step(st, x, u, status, npts, om, v_used, ep["flag"] == 0, ss, new_count=int(gone.sum()), max_total=npts)
        kept = int((~gone).sum())
        out.append(dict(v_epi=ep["v"].copy(), v_plain=v_plain, v_map=rec[0:3].copy(), flag=int(rec[3]), mature=int(rec[4]), rec=rec, epi_flag=ep["flag"],
                        rho_true=rho.copy(), z=diag["z"], rho_prior=prior["rho"], var_prior=prior["var"], nobs_prior=prior["nobs"],
                        rho_post=st["rho"][:kept].copy(), var_post=st["var"][:kept].copy(), nobs_post=st["nobs"][:kept].copy(),
                        rho_next=rho_next[~gone]))
        # the plane of the next frame: P+ = A P + v
        n2 = Ai.T @ nrm; ln = np.linalg.norm(n2)
        d = (d + nrm @ (Ai @ v)) / ln; nrm = n2 / ln
        stay = x_next[~gone]
        xb, rb, lb = _born(npts - kept, d, nrm, rng, max(0, FOOT_POINTS - int((np.hypot(stay[:, 0], stay[:, 1]) <= er.FOOT).sum())))
        x = np.concatenate([stay, xb]); rho = np.concatenate([rho_next[~gone], rb]); level = np.concatenate([level[~gone], lb])
    return out


def rel_err(v, truth=er.V):
    return float(np.linalg.norm(np.asarray(v) - truth) / np.linalg.norm(truth))
