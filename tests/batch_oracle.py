"""The CPU oracle chain of one frame pair (gray -> corners -> pyramidal LK -> node solve -> lever arm and rotation), run over many
pairs on a thread pool, the same chain with the corner grid and with every pair setting composed, and the comparisons the batch-shape GPU tests apply to ofk_pairs_run's outputs.  Test infrastructure only."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import image_oracle as io, estimation_oracle as eo

THREADS = 16                     # the C image stages release the GIL; a fixed pool, not one sized by the host's CPU count


def oracle_chain(prev, nxt, cfg, sr):
    """io.gray_bgr8 -> io.good_features -> io.lk_pyr -> eo.solve_lgs_node + eo.post_solve for one pair, sensors row `sr`.
    Zero corners (or zero tracked points) give what the device's solve guard writes: v = s = 0, rank 0."""
    g0, g1 = io.gray_bgr8(prev), io.gray_bgr8(nxt)
    pts = io.good_features(g0, cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size)
    n, s, e = io.lk_pyr(g0, g1, pts, cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr)
    ok = s.ravel() == 1
    d, nrm, om = sr[0], sr[1:4], sr[4:7]
    sc, cx, cy = sr[19], sr[20], sr[21]
    new = n.reshape(-1, 2).astype(np.float64); old = pts.reshape(-1, 2).astype(np.float64)
    x = (new[ok] - [cx, cy]) * sc; u = (new[ok] - old[ok]) * sc
    if len(x):
        v, R, rank, sv = eo.solve_lgs_node(x, u, d, nrm, om)
    else:
        v, R, rank, sv = np.zeros(3), np.zeros(0), 0, np.zeros(3)
    v_uav = eo.post_solve(v, sr[7:16].reshape(3, 3), om, sr[16:19])
    return dict(pts=pts.reshape(-1, 2), nxt=n.reshape(-1, 2), status=s.ravel(), err=e.ravel(), v=v, R=R, rank=int(rank), s=sv,
                v_uav=v_uav, used=len(x), tracked=int(ok.sum()))


def grid_chain(prev, nxt, cfg, sr, grid):
    """oracle_chain with the corners taken from the corner grid's reference selection (tests/corner_grid_reference.py)."""
    import corner_grid_reference as R
    g0, g1 = io.gray_bgr8(prev), io.gray_bgr8(nxt)
    pts, stats, _ = R.good_features(g0, cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size, grid=grid)
    n, s, e = io.lk_pyr(g0, g1, pts.reshape(-1, 1, 2), cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr)
    ok = s.ravel() == 1
    new = n.reshape(-1, 2).astype(np.float64); old = pts.astype(np.float64)
    x = (new[ok] - [sr[20], sr[21]]) * sr[19]; u = (new[ok] - old[ok]) * sr[19]
    v, Rr, rank, sv = eo.solve_lgs_node(x, u, sr[0], sr[1:4], sr[4:7])
    return dict(pts=pts, nxt=n.reshape(-1, 2), status=s.ravel(), err=e.ravel(), v=v, R=Rr, rank=int(rank), s=sv,
                v_uav=eo.post_solve(v, sr[7:16].reshape(3, 3), sr[4:7], sr[16:19]), used=len(x), tracked=int(ok.sum()), stats=stats,
                plain=io.good_features(g0, cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size).reshape(-1, 2))


def combined_chain(prev, nxt, cfg, sr, problem, grid, gate, seed_mode, robust, cov, gain=1.0, predict=None):
    """One frame pair with the settings composed as ofk_pairs_run composes them: the grid's selection (corner_grid_reference) -> the
    seeded forward pass and the gates (track_gate_reference.gated_cfg with seed= and flags=) -> the robust solve on the gated status
    (robust_reference; `problem` = the pair's index in the batch, it picks the sample) -> the covariance behind it (cov_reference).
    robust: robust_reference.robust_solve's keywords; cov: cov_reference.pair_record's cfg.  predict(pts, sr, mode, gain) puts
    another seed predictor in the place of lk_seed_reference.predict.  A dict assert_pair_matches accepts, plus gate, weights,
    robust (the solve's full result), grid_stats and cov (the 24-double record)."""
    import corner_grid_reference as CG
    import cov_reference as CR
    import lk_seed_reference as LS
    import robust_reference as RR
    import track_gate_reference as TG
    g0, g1 = io.gray_bgr8(prev), io.gray_bgr8(nxt)
    pts, stats, _ = CG.good_features(g0, cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size, grid=grid)
    if seed_mode and len(pts):
        seed = np.ascontiguousarray((predict or LS.predict)(pts, sr, seed_mode, gain), np.float32).reshape(-1, 2)
        r = TG.gated_cfg(g0, g1, pts, cfg, gate, seed=seed, flags=LS.USE_INITIAL_FLOW)
    else:
        r = TG.gated_cfg(g0, g1, pts, cfg, gate)
    ok = r["keep"]
    new = r["next"].astype(np.float64); old = pts.astype(np.float64)
    x = (new - [sr[20], sr[21]]) * sr[19]; u = (new - old) * sr[19]
    rb = RR.robust_solve(RR.NODE, x, u, sr[0], sr[1:4], sr[4:7], valid=ok, problem=problem, **robust)
    rec = np.zeros(16); rec[0:3] = rb["v"]; rec[3] = rb["r"]; rec[4] = rb["rank"]
    cv = CR.pair_record(CR.NODE, pts, r["next"], r["status"], sr, cov, rec, w=rb["weights"])
    return dict(pts=pts, nxt=r["next"], status=r["status"], err=r["err"], v=rb["v"], R=np.array([rb["r"]]), rank=int(rb["rank"]), s=rb["s"],
                v_uav=eo.post_solve(rb["v"], sr[7:16].reshape(3, 3), sr[4:7], sr[16:19]), used=int(rb["cnt"]), tracked=int(ok.sum()),
                gate=r, weights=rb["weights"], robust=rb, grid_stats=stats, cov=cv)


def oracle_many(prev, nxt, cfg, sensors, idx):
    """oracle_chain of the pairs `idx` on THREADS threads -> {pair: result}."""
    idx = [int(b) for b in idx]
    with ThreadPoolExecutor(min(THREADS, max(1, len(idx)))) as ex:
        res = list(ex.map(lambda b: oracle_chain(prev[b], nxt[b], cfg, sensors[b]), idx))
    return dict(zip(idx, res))


def assert_pair_matches(out, b, ref, what=""):
    """Pair b of an ofk_pairs_download result against oracle_chain: corners, status, next points and err bit for bit (floats as
    uint32), the velocity records at the suite's tolerances, rank / used / count / tracked exactly."""
    tag = f"pair {b} {what}"
    n = int(out["counts"][b])
    assert n == len(ref["pts"]), (tag, n, len(ref["pts"]))
    assert np.array_equal(out["prev_pts"][b, :n].view(np.uint32), ref["pts"].view(np.uint32)), tag
    assert np.array_equal(out["status"][b, :n], ref["status"]), tag
    assert np.array_equal(out["next_pts"][b, :n].view(np.uint32), ref["nxt"].view(np.uint32)), tag
    assert np.array_equal(out["err"][b, :n].view(np.uint32), ref["err"].view(np.uint32)), tag
    rec = out["records"][b]
    assert rec[4] == ref["rank"] and rec[11] == ref["used"] and rec[12] == n and rec[13] == ref["tracked"], (tag, rec[[4, 11, 12, 13]], ref["rank"], ref["used"], ref["tracked"])
    np.testing.assert_allclose(rec[0:3], ref["v"], rtol=1e-9, atol=1e-13, err_msg=tag)
    np.testing.assert_allclose(rec[5:8], ref["s"], rtol=1e-9, err_msg=tag)
    np.testing.assert_allclose(rec[8:11], ref["v_uav"], rtol=1e-9, atol=1e-13, err_msg=tag)
    if ref["R"].size:
        np.testing.assert_allclose(rec[3], ref["R"][0], rtol=1e-6, atol=1e-18, err_msg=tag)


def assert_records_identical(a, b, what=""):
    """Two GPU runs' records bit for bit (uint64 views: NaN and zero-corner records compare too)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.argwhere(a.view(np.uint64) != b.view(np.uint64))
    assert bad.size == 0, (what, bad[:6])
