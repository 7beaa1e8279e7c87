"""Test-side reference of the track gates (include/ofk.h: ofk_set_track_gate, ofk_lk_pyr_fb): the forward-backward check and the
cap on LK's err, rule by rule in numpy over tests/lk_seed_reference.lk_pyr for both passes.

gate         a dict(fb="off"|"plain"|"seeded", fb_thr, fb_level, err_max) - the keywords of ofk.track_gate_setting.
gated        the five rules for one image -> dict(next, status, st_f, err, back, st_b, fb2, stats, keep).
gated_lk     the tracker plug lk(g_prev, g, old) of stream_oracle.NodeLoop.
seeded_gated_lk  the tracker plug lk(g_prev, g, old, src) of stream_oracle.NodeLoop (lk_src=): the gates over the seeded forward pass.
gated_chain  batch_oracle.oracle_chain with the gate between LK and the solve (a dict batch_oracle.assert_pair_matches accepts).
experiment   the rows of lk_seed_reference.ROWS gated: tracked / wrong / good-lost counts and the NODE solve's relative error.
"""
import numpy as np

from oracle import image_oracle as io, estimation_oracle as eo
import lk_seed_reference as R  # tests/lk_seed_reference.py

OFF = dict(fb="off", fb_thr=0.5, fb_level=-1, err_max=0.0)


def setting(fb="off", fb_thr=0.5, fb_level=-1, err_max=0.0):
    return dict(fb=fb, fb_thr=float(fb_thr), fb_level=int(fb_level), err_max=float(err_max))


def back_level(gate, max_level):
    """maxLevel of the backward pass: -1 = the forward pass's, else min(fb_level, forward maxLevel)."""
    return max_level if gate["fb_level"] < 0 else min(gate["fb_level"], max_level)


def gated(g0, g1, pts, win, max_level, max_count, eps, min_eig_thr, gate, seed=None, flags=0):
    """Rules 1-5 of ofk.h for the points of one image.  seed / flags: the forward pass's (lk_seed_reference.lk_pyr)."""
    p = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = len(p)
    if n == 0:
        z2, z1 = np.zeros((0, 2), np.float32), np.zeros(0, np.float32)
        zb = np.zeros(0, np.uint8)
        return dict(next=z2, status=zb, st_f=zb, err=z1, back=z2, st_b=zb, fb2=z1, stats=np.zeros(4, np.int32), keep=np.zeros(0, bool))
    # 1. the forward pass
    nxt, st, err = R.lk_pyr(g0, g1, p, win, max_level, max_count, eps, min_eig_thr, seed=seed, flags=flags)
    nxt = nxt.reshape(-1, 2); st_f = st.ravel() == 1; err = err.ravel()
    fb_on = gate["fb"] != "off"
    back = np.zeros((n, 2), np.float32); st_b = np.ones(n, bool); fb2 = np.full(n, np.inf, np.float32)
    over = np.zeros(n, bool)
    if fb_on:
        # 2. the backward pass: the pyramids swapped, from next[i] for every point, whatever st_f is
        lb = back_level(gate, max_level)
        if gate["fb"] == "seeded":
            bk, sb, _ = R.lk_pyr(g1, g0, nxt, win, lb, max_count, eps, min_eig_thr, seed=p, flags=R.USE_INITIAL_FLOW)
        else:
            bk, sb, _ = R.lk_pyr(g1, g0, nxt, win, lb, max_count, eps, min_eig_thr)
        back = bk.reshape(-1, 2); st_b = sb.ravel() == 1
        # 3. the distance, float32 operation by operation
        with np.errstate(all="ignore"):
            dx = back[:, 0] - p[:, 0]; dy = back[:, 1] - p[:, 1]
            d2 = (dx * dx + dy * dy).astype(np.float32)
            both = st_f & st_b
            fb2 = np.where(both, d2, np.float32(np.inf)).astype(np.float32)
            thr2 = np.float32(gate["fb_thr"] * gate["fb_thr"])            # squared in double, rounded once
            over = both & ~(d2 <= thr2)
    # 4. the keep rule
    capped = np.zeros(n, bool)
    if gate["err_max"] != 0.0:
        with np.errstate(all="ignore"):
            capped = ~(err <= np.float32(gate["err_max"]))
    lost_b = st_f & ~st_b
    far = st_f & st_b & over
    cap = st_f & st_b & ~over & capped
    keep = st_f & st_b & ~over & ~capped
    stats = np.array([st_f.sum(), lost_b.sum(), far.sum(), cap.sum()], np.int32)
    # 5. status := keep; next and err as the forward pass left them
    return dict(next=nxt, status=keep.astype(np.uint8), st_f=st_f.astype(np.uint8), err=err, back=back, st_b=st_b.astype(np.uint8),
                fb2=fb2, stats=stats, keep=keep)


def gated_cfg(g0, g1, pts, cfg, gate, seed=None, flags=0):
    return gated(g0, g1, pts, cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr, gate, seed=seed, flags=flags)


def gated_lk(cfg, gate, log=None):
    """The tracker plug of NodeLoop: (next, gated status, err).  log (a list) receives every call's full result."""
    def lk(g_prev, g, old):
        r = gated_cfg(g_prev, g, old, cfg, gate)
        if log is not None:
            log.append(r)
        return r["next"].reshape(-1, 1, 2), r["status"].reshape(-1, 1), r["err"].reshape(-1, 1)
    return lk


def seeded_gated_lk(cfg, gate, mode, gain=1.0, log=None, predict=None):
    """NodeLoop's lk_src plug under ofk_set_lk_seed + ofk_set_track_gate: the forward pass starts at the seeds predicted from the
    row `src` (lk_seed_reference.predict; mode 0 = unseeded), the gates follow.  predict(old, src, mode, gain) -> seeds [n,2] f32
    puts another predictor in its place (the device's ofk_predict_points).  log (a list) receives every call's full result."""
    def lk(g_prev, g, old, src):
        if mode and len(old):
            seed = np.ascontiguousarray((predict or R.predict)(old, src, mode, gain), np.float32).reshape(-1, 2)
            r = gated_cfg(g_prev, g, old, cfg, gate, seed=seed, flags=R.USE_INITIAL_FLOW)
        else:
            r = gated_cfg(g_prev, g, old, cfg, gate)
        if log is not None:
            log.append(r)
        return r["next"].reshape(-1, 1, 2), r["status"].reshape(-1, 1), r["err"].reshape(-1, 1)
    return lk


def gated_chain(prev, nxt, cfg, sr, gate):
    """batch_oracle.oracle_chain with the gate between LK and the solve; the gate's own outputs ride along under "gate"."""
    g0, g1 = io.gray_bgr8(prev), io.gray_bgr8(nxt)
    pts = io.good_features(g0, cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size).reshape(-1, 2)
    r = gated_cfg(g0, g1, pts, cfg, gate)
    ok = r["keep"]
    d, nrm, om = sr[0], sr[1:4], sr[4:7]
    sc, cx, cy = sr[19], sr[20], sr[21]
    new = r["next"].astype(np.float64); old = pts.astype(np.float64)
    x = (new[ok] - [cx, cy]) * sc; u = (new[ok] - old[ok]) * sc
    if len(x):
        v, Rs, rank, sv = eo.solve_lgs_node(x, u, d, nrm, om)
    else:
        v, Rs, rank, sv = np.zeros(3), np.zeros(0), 0, np.zeros(3)
    v_uav = eo.post_solve(v, sr[7:16].reshape(3, 3), om, sr[16:19])
    return dict(pts=pts, nxt=r["next"], status=r["status"], err=r["err"], v=v, R=Rs, rank=int(rank), s=sv, v_uav=v_uav, used=len(x),
                tracked=int(ok.sum()), gate=r)


# ---------------------------------------------------------------------------------------- the experiment of the issue's table
EXP_THR = 0.5
EXP_LEVEL = 3
VARIANTS = (("plain L3", dict(fb="plain", fb_level=-1)), ("seeded L3", dict(fb="seeded", fb_level=-1)),
            ("seeded L0", dict(fb="seeded", fb_level=0)))


def node_rel_error(e, nxt, keep):
    """Relative error of the NODE solve on the kept points of an experiment row (x = new position, u = new - old)."""
    pair = e["pair"]
    s = R.experiment_sensors(pair)
    new = nxt[keep].astype(np.float64); old = e["pts"][keep].astype(np.float64)
    x = (new - [s[20], s[21]]) * s[19]; u = (new - old) * s[19]
    v = eo.solve_lgs_node(x, u, s[0], s[1:4], s[4:7])[0]
    return float(np.linalg.norm(v - pair["v"]) / np.linalg.norm(pair["v"]))


def experiment_row(name):
    """-> dict(tracked, wrong, good, rel) ungated and per variant dict(kept, wrong, lost, rel) over all corners of the row."""
    e = R.experiment_pair(name)
    end = e["pts"].astype(np.float64) + e["flow"]
    out = {}
    for label, kw in (("ungated", dict(fb="off")),) + VARIANTS:
        r = gated(e["g0"], e["g1"], e["pts"], max_level=EXP_LEVEL, gate=setting(fb_thr=EXP_THR, **kw), **R.EXP_LK)
        dist = np.linalg.norm(r["next"].astype(np.float64) - end, axis=1)
        right = (r["st_f"] == 1) & (dist <= 0.5)
        keep = r["keep"]
        out[label] = dict(kept=int(keep.sum()), wrong=int((keep & ~right).sum()), good=int(right.sum()), lost=int((right & ~keep).sum()),
                          rel=node_rel_error(e, r["next"], keep) if keep.sum() >= 3 else float("nan"))
    return out
