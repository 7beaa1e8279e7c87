"""CPU-only: pins tests/robust_reference.py itself - without hypotheses and rounds it is the oracle's plain solve; exact data with up
to 45 % arbitrary outliers give the true velocity back with flag 2; fewer than 8 points give flag 1; and the moving-object experiment on
the CPU oracle chain meets its two conditions in every scene (the figures are printed: they are the ones robust_reference.py quotes)."""
import numpy as np
import pytest

import robust_reference as rr
from oracle import estimation_oracle as eo, image_oracle as io

SC = 1.0 / 640.0


def exact_problem(rng, n, share):
    x = rng.uniform(-0.45, 0.45, (n, 2)) * np.array([1.0, 0.75])
    v = rng.uniform(-0.005, 0.005, 3); om = rng.uniform(-0.004, 0.004, 3)
    d = rng.uniform(0.8, 1.5); nrm = np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), 1.0]); nrm /= np.linalg.norm(nrm)
    u = eo.generate_test_data(x, v, om, d, nrm)
    out = rng.permutation(n)[:int(share * n)]
    u[out] += rng.uniform(-20, 20, (len(out), 2)) * SC
    return x, u, v, om, d, nrm, out


def test_without_hypotheses_and_rounds_it_is_the_plain_solve():
    rng = np.random.default_rng(1)
    for n in (3, 8, 50, 500):
        x, u, v, om, d, nrm, _ = exact_problem(rng, n, 0.2)
        u += rng.standard_normal(u.shape) * 0.05 * SC
        t = rng.uniform(-0.1, 0.1, 3); dist = rng.uniform(0.5, 2.0, n)
        ref = eo.solve_lgs_node(x, u, d, nrm, om)
        r = rr.robust_solve(rr.NODE, x, u, d, nrm, om, hypotheses=0, iters=0)
        np.testing.assert_allclose(r["v"], ref[0], rtol=1e-9, atol=1e-13)
        np.testing.assert_allclose(r["s"], ref[3], rtol=1e-9)
        assert r["rank"] == ref[2] and np.array_equal(r["weights"], np.ones(n)) and r["stats"][6] == 0
        if n > 3:
            np.testing.assert_allclose(r["r"], ref[1][0], rtol=1e-6)
        vs, Rs, ss = eo.solve_lgs_sim(x, u, d, nrm, om, t)
        r = rr.robust_solve(rr.SIM, x, u, d, nrm, om, hypotheses=0, iters=0)
        np.testing.assert_allclose(r["v"] - np.cross(om, t), vs, rtol=1e-9, atol=1e-13)
        np.testing.assert_allclose(r["s"], ss, rtol=1e-9)
        x3 = np.concatenate([x, np.ones((n, 1))], 1); u3 = np.concatenate([u, np.zeros((n, 1))], 1)
        vo = eo.solve_of_module(x3, u3, dist, nrm)
        r = rr.robust_solve(rr.OFMODULE, x, u, None, nrm, None, wgt=dist, hypotheses=0, iters=0)
        np.testing.assert_allclose(r["v"], vo[0], rtol=1e-9, atol=1e-13)
        np.testing.assert_allclose(r["s"], vo[3], rtol=1e-9)


@pytest.mark.parametrize("loss", (rr.HUBER, rr.TUKEY))
@pytest.mark.parametrize("variant", (rr.NODE, rr.SIM))
def test_exact_data_with_outliers_returns_the_truth(loss, variant):
    rng = np.random.default_rng(10 * loss + variant)
    worst = 0.0
    for n in (8, 9, 20, 64, 257, 500):
        for share in (0.0, 0.2, 0.45):
            x, u, v, om, d, nrm, out = exact_problem(rng, n, share)
            r = rr.robust_solve(variant, x, u, d, nrm, om, loss=loss, c=4.685 if loss == rr.TUKEY else 1.345, iters=5, hypotheses=256, seed=n)
            assert r["stats"][7] == 2 and r["stats"][6] == 0 and r["stats"][4] >= 0, (n, share, r["stats"])
            assert np.array_equal(r["weights"], np.ones(n))
            np.testing.assert_allclose(r["v"], v, rtol=1e-9, atol=1e-12)
            worst = max(worst, float(np.abs(r["v"] - v).max()))
    print("largest error on exact data", worst)


def test_few_points_give_flag_1():
    rng = np.random.default_rng(3)
    x, u, v, om, d, nrm, _ = exact_problem(rng, 40, 0.0)
    for m in (0, 1, 3, 7):
        valid = np.zeros(40, bool); valid[rng.permutation(40)[:m]] = True
        r = rr.robust_solve(rr.NODE, x, u, d, nrm, om, valid=valid)
        assert r["stats"][7] == 1 and r["stats"][3] == m and r["stats"][4] == -1 and np.array_equal(r["weights"], valid.astype(float))
        if m >= 3:
            np.testing.assert_allclose(r["v"], eo.solve_lgs_node(x[valid], u[valid], d, nrm, om)[0], rtol=1e-9, atol=1e-13)
    valid = np.zeros(40, bool); valid[:8] = True
    assert rr.robust_solve(rr.NODE, x, u, d, nrm, om, valid=valid)["stats"][7] != 1


def test_sample_is_philox():
    # Random123's known answer for the all-zero counter and key pins the generator the sample comes from
    x = eo.philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(v) for v in x] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    i, j = rr.sample(0, 0, 1, 1000)
    assert (int(i[0]), int(j[0])) == (0x6627E8D5 % 1000, (0xE169C58D % 999) + ((0xE169C58D % 999) >= (0x6627E8D5 % 1000)))


def test_moving_object_experiment_on_the_cpu_chain(pkg):
    from of_amd import synth
    from of_amd.pipeline import PipelineConfig
    cfg = PipelineConfig(max_corners=300, quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)
    for size in rr.OBJECT_SIZES + (None,):
        plain, robust, share, left = [], [], [], []
        for seed in rr.SCENE_SEEDS:
            pair, prev, nxt = rr.scene(synth, seed, size)
            g0, g1 = io.gray_bgr8(prev), io.gray_bgr8(nxt)
            pts = io.good_features(g0, cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size)
            n, s, e = io.lk_pyr(g0, g1, pts, cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr)
            ok = s.ravel() == 1
            new = n.reshape(-1, 2).astype(np.float64); old = pts.reshape(-1, 2).astype(np.float64)
            x = (new - [pair["cx"], pair["cy"]]) * pair["scaling"]; u = (new - old) * pair["scaling"]
            vp = eo.solve_lgs_node(x[ok], u[ok], pair["d"], pair["n"], pair["omega"])[0]
            r = rr.robust_solve(rr.NODE, x, u, pair["d"], pair["n"], pair["omega"], valid=ok, **rr.EXPERIMENT)
            obj = rr.on_object(old, size) & ok
            plain.append(rr.rel_err(vp, pair["v"])); robust.append(rr.rel_err(r["v"], pair["v"]))
            share.append(obj.sum() / ok.sum()); left.append(int(np.count_nonzero(r["weights"][obj] > 0)))
            assert r["gap"] >= 1e-6 and r["near"] == 0                # what the device comparison presupposes
            rr.check_experiment(size, plain[-1], robust[-1], (size, seed))
        print(f"object {size}: share {min(share):.2f}-{max(share):.2f} plain {min(plain):.4f}-{max(plain):.4f} "
              f"robust {min(robust):.4f}-{max(robust):.4f} object corners with w > 0: {left}")


def test_drop_removes_the_object_from_the_tracks_of_the_restated_loop(pkg):
    """What `drop` achieves, on the CPU loop: the share of tracks on the moving object after the last frame is strictly smaller
    with it (the figures robust_stream_oracle.py quotes)."""
    from of_amd import synth, ofk
    from of_amd.pipeline import PipelineConfig
    import robust_stream_oracle as rso
    from stream_oracle import NodeLoop
    h, w, nf = 480, 640, 6
    cfg = PipelineConfig(max_corners=200, quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)
    for seed in (900, 901):
        frames, info = rso.sequence(synth, h, w, seed, nf)
        sr = ofk.make_sensors(1, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"])[0]
        share = {}
        for drop in (False, True):
            loop = NodeLoop(frames[0], cfg, 150, 15, solve=rso.robust_solver(0, drop, False))
            for t in range(1, nf):
                out = loop.step(frames[t], sr)
                assert rr.rel_err(out["v"], info["v"]) <= rr.ROBUST_MAX, (seed, drop, t)
            share[drop] = float(np.mean(rso.on_object(out["tracks"], nf - 1))) if len(out["tracks"]) else 0.0
        print(f"seed {seed}: share of tracks on the object after the last frame: drop off {share[False]:.3f}, drop on {share[True]:.3f}")
        assert share[True] < share[False]
