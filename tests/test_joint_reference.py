"""CPU-only: the joint velocity and rotation solve of ofk.h (ofk_set_joint) as tests/joint_reference.py restates it - against an
independent stacked least squares, at its flags, and on the experiment that motivates it.

TOL, the tolerance the GPU tests hold the device to as well, is pinned here: 16 x the largest relative deviation of (v, omega^)
between the restatement (normal equations, Schur complement, the kernel's summation order) and np.linalg.lstsq on the stacked
3 m + 3 rows over every case below (the convention of tests/estimation_edge_cases.py).  Measured: 5.8e-14 (257 points, SIM, free, robust weights).

The experiment (experiment_scenes(): 400 points over 1280 x 960, f = 1000, d = 1.5, v = (0.02, -0.015, 0.004) and omega = (0.004,
-0.003, 0.01) per frame, 0.2 px of flow noise, gyro error e (1, -1, 0.5), generator seed 3), relative error of v, measured with the
committed code:
    e        plain     joint, free   joint, sigma 1e-3   joint, sigma 1e-4
    0        0.0019    0.0040        0.0040              0.0027
    3e-4     0.0284    0.0040        0.0040              0.0116
    1e-3     0.0926    0.0040        0.0042              0.0371
    3e-3     0.2761    0.0040        0.0047              0.1104
The free omega^ is within 5.5e-5 of the truth; with the scene's 50 points the free column is 0.024.
The rendered 480 x 640 pair (synth.render_pair, seeds 20-23, sensor omega off by 1e-3 (1, -1, 0.5)) through the C oracle chain: plain
0.27, joint 0.06-0.10; the figures are in test_rendered_pair_through_the_oracle_chain's docstring."""
import numpy as np
import pytest

import joint_reference as jr
from oracle import estimation_oracle as eo

TOL = 16 * 5.8e-14                                              # 16 x the measured 5.8e-14, see above
MEASURED = dict(dev=0.0)


def deviation(n, variant, prior, weights):
    x, u, d, nrm, om0, v, om = jr.scene(n, 1000 + n, outliers=weights)
    w = jr.robust_weights(variant, x, u, d, nrm, om0) if weights else None
    if weights and n >= 64:
        assert np.any((w > 0) & (w < 1))                         # real weights, not all ones
    got = jr.joint_solve(variant, x, u, d, nrm, om0, jr.SIGMA_FLOW, prior, w=w)
    assert got["flag"] == 0 and got["rewritten"], (n, variant, prior)
    vl, ol = jr.joint_lstsq(variant, x, u, d, nrm, om0, jr.SIGMA_FLOW, prior, w=w)
    return jr.rel_dev(got["v"], got["omega"], vl, ol)


@pytest.mark.parametrize("n", jr.COUNTS)
def test_restatement_against_stacked_lstsq(n):
    for variant in (jr.NODE, jr.SIM):
        for name, prior in jr.PRIORS.items():
            for weights in (False, True):
                dev = deviation(n, variant, prior, weights)
                MEASURED["dev"] = max(MEASURED["dev"], dev)
                assert dev <= TOL, (n, variant, name, weights, dev)
    print(f"n {n}: largest relative deviation of (v, omega^) so far {MEASURED['dev']:.3e}")


@pytest.mark.parametrize("variant", (jr.NODE, jr.SIM))
def test_exact_flow_returns_the_truth(variant):
    for n in (3, 65, 400):
        x, u, d, nrm, om0, v, om = jr.scene(n, 7 + n, noise=0.0)
        assert np.abs(om0 - om).max() == 3e-3
        got = jr.joint_solve(variant, x, u, d, nrm, om0, jr.SIGMA_FLOW, jr.PRIORS["free"])
        assert got["flag"] == 0
        assert np.abs(got["v"] - v).max() <= 1e-12 and np.abs(got["omega"] - om).max() <= 1e-12, (n, got["v"] - v, got["omega"] - om)
        assert got["rss"] <= 1e-24
        plain = jr.plain_solve(variant, x, u, d, nrm, om0)[0]
        assert np.linalg.norm(plain - v) / np.linalg.norm(v) > 0.05       # what the wrong gyro costs the plain solve here


def test_all_axes_held_is_the_plain_solve():
    x, u, d, nrm, om0, v, om = jr.scene(257, 3)
    vs, rss, rank = jr.plain_solve(jr.NODE, x, u, d, nrm, om0)
    got = jr.joint_solve(jr.NODE, x, u, d, nrm, om0, jr.SIGMA_FLOW, (0.0, 0.0, 0.0))
    assert got["flag"] == 0 and not got["rewritten"]
    assert np.array_equal(got["v"].view(np.uint64), vs.view(np.uint64)) and np.array_equal(got["omega"], om0) and got["rss"] == rss
    rec = got["rec"]
    assert np.all(rec[3:6] == 0) and np.all(rec[12:21] == 0) and np.all(rec[21:27] != 0)
    # one axis held: its delta is exactly 0 and the other two equal the stacked solve without that column
    got = jr.joint_solve(jr.NODE, x, u, d, nrm, om0, jr.SIGMA_FLOW, (np.inf, 0.0, np.inf))
    assert got["rec"][4] == 0.0 and got["rec"][14] == 0.0 and got["rec"][13] > 0.0
    vl, ol = jr.joint_lstsq(jr.NODE, x, u, d, nrm, om0, jr.SIGMA_FLOW, (np.inf, 0.0, np.inf))
    assert jr.rel_dev(got["v"], got["omega"], vl, ol) <= TOL


def test_collinear_points_are_unobservable():
    x, u, d, nrm, om0, v, om = jr.scene(20, 5, noise=0.0)
    s = np.linspace(-0.5, 0.5, 20)
    x = np.stack([s, 0.3 * s + 0.1], 1)
    u = eo.generate_test_data(x, v, om, d, nrm)
    vs, rss, rank = jr.plain_solve(jr.NODE, x, u, d, nrm, om0)
    assert rank == 3                                            # the velocity alone is observable on a line
    got = jr.joint_solve(jr.NODE, x, u, d, nrm, om0, jr.SIGMA_FLOW, jr.PRIORS["free"])
    assert got["flag"] == 2 and got["rec"][10] == 2.0 and not got["rewritten"]
    assert np.array_equal(got["v"], vs) and np.array_equal(got["omega"], om0) and np.all(got["rec"][3:6] == 0) and np.all(got["rec"][15:27] == 0)
    assert got["rec"][12] > 0 and got["rec"][14] < np.sqrt(jr.EPS * 60) * got["rec"][12]
    assert jr.joint_solve(jr.NODE, x, u, d, nrm, om0, jr.SIGMA_FLOW, jr.PRIORS["prior"])["flag"] == 0      # a prior makes it a problem again


def test_not_attempted():
    x, u, d, nrm, om0, v, om = jr.scene(8, 6)
    one = jr.joint_solve(jr.NODE, x[:1], u[:1], d, nrm, om0, jr.SIGMA_FLOW, jr.PRIORS["free"])
    assert one["flag"] == 1 and one["rec"][10] == 1.0 and one["rec"][11] == 1 and np.array_equal(one["rec"][0:3], om0)
    nan = jr.joint_solve(jr.NODE, x, u, np.nan, nrm, om0, jr.SIGMA_FLOW, jr.PRIORS["free"])
    assert nan["flag"] == 1 and np.array_equal(nan["v"], np.zeros(3)) and np.array_equal(nan["rec"][0:3], om0)
    zero = jr.joint_solve(jr.SIM, x, u, 0.0, nrm, om0, jr.SIGMA_FLOW, jr.PRIORS["free"])
    assert zero["flag"] == 1 and not zero["rewritten"]
    none = jr.joint_solve(jr.NODE, x, u, d, nrm, om0, jr.SIGMA_FLOW, jr.PRIORS["free"], valid=np.zeros(8, np.uint8))
    assert none["flag"] == 1 and none["rec"][11] == 0


ERRORS = (0.0, 3e-4, 1e-3, 3e-3)
# recorded with the committed code (the module docstring's table): plain, free, sigma 1e-3 per gyro error
RECORDED = {0.0: (0.0019, 0.0040, 0.0040), 3e-4: (0.0284, 0.0040, 0.0040), 1e-3: (0.0926, 0.0040, 0.0042), 3e-3: (0.2761, 0.0040, 0.0047)}


def experiment_scenes():
    """The experiment's scenes, one generator (seed 3) drawn from in this order: 50 points, then 400, uniform over a 1280 x 960 frame
    less a 40 px border, f = 1000; per count the scene's points, then its 0.2 px flow noise.  {count: (x, u)}."""
    rng = np.random.default_rng(3)
    out = {}
    for N in (50, 400):
        px = np.stack([rng.uniform(40, 1280 - 40, N), rng.uniform(40, 960 - 40, N)], -1)
        x = (px - [640.0, 480.0]) / 1000.0
        out[N] = (x, eo.generate_test_data(x, EXP_V, EXP_OM, EXP_D, EXP_N) + rng.normal(0, 2e-4, (N, 2)))
    return out


EXP_V, EXP_OM, EXP_D = np.array([0.02, -0.015, 0.004]), np.array([0.004, -0.003, 0.01]), 1.5
EXP_N = np.array([0.05, -0.03, 1.0]) / np.linalg.norm([0.05, -0.03, 1.0])


def table(N=400):
    """Relative error of v: {e: (plain, free, sigma 1e-3, sigma 1e-4)}; the largest error of the free omega^ rides along."""
    x, u = experiment_scenes()[N]
    out = {}
    worst = 0.0
    for e in ERRORS:
        om0 = EXP_OM + e * np.array([1.0, -1.0, 0.5])
        errs = [np.linalg.norm(eo.solve_lgs_node(x, u, EXP_D, EXP_N, om0)[0] - EXP_V)]
        for so in (np.inf, 1e-3, 1e-4):
            got = jr.joint_solve(jr.NODE, x, u, EXP_D, EXP_N, om0, 2e-4, (so,) * 3)
            assert got["flag"] == 0
            errs.append(np.linalg.norm(got["v"] - EXP_V))
            if so == np.inf:
                worst = max(worst, np.abs(got["omega"] - EXP_OM).max())
        out[e] = tuple(np.array(errs) / np.linalg.norm(EXP_V))
    return out, worst


def test_gyro_error_experiment():
    got, worst = table()
    few, _ = table(50)
    print(f"free omega^ within {worst:.2e} of the truth; with 50 points the free column is {few[1e-3][1]:.4f}")
    assert worst < 3 * 5.5e-5                                    # recorded: 5.5e-5
    for e in ERRORS:
        print(f"e {e:g}: plain {got[e][0]:.4f}  free {got[e][1]:.4f}  sigma 1e-3 {got[e][2]:.4f}  sigma 1e-4 {got[e][3]:.4f}")
        plain, free, prior = RECORDED[e]
        if e > 0:
            assert got[e][0] >= plain / 3, (e, "plain", got[e][0])
        assert got[e][1] <= 3 * free and got[e][2] <= 3 * prior, (e, got[e])
    assert got[1e-3][0] > 10 * got[1e-3][1]                      # 0.093 against 0.004
    assert got[0.0][1] <= 3 * got[0.0][0] and got[0.0][2] <= 3 * got[0.0][0]


RENDER_SEEDS = (20, 21, 22, 23)


def rendered(pkg_synth, PipelineConfig, io):
    cfg = PipelineConfig(max_corners=300, quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)
    rows = []
    for seed in RENDER_SEEDS:
        pair = pkg_synth.render_pair(480, 640, seed, margin=96, v=(0.004, -0.003, 0.002), omega=(0.003, -0.002, 0.004), d=1.0)
        g0, g1 = io.gray_bgr8(pair["prev"]), io.gray_bgr8(pair["next"])
        pts = io.good_features(g0, cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size)
        n, s, e = io.lk_pyr(g0, g1, pts, cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr)
        ok = s.ravel() == 1
        new = n.reshape(-1, 2).astype(np.float64); old = pts.reshape(-1, 2).astype(np.float64)
        x = (new - [pair["cx"], pair["cy"]]) * pair["scaling"]; u = (new - old) * pair["scaling"]
        om0 = np.asarray(pair["omega"], np.float64) + 1e-3 * np.array([1.0, -1.0, 0.5])
        truth = np.asarray(pair["v"], np.float64)
        exact = np.linalg.norm(eo.solve_lgs_node(x[ok], u[ok], pair["d"], pair["n"], pair["omega"])[0] - truth) / np.linalg.norm(truth)
        plain = np.linalg.norm(eo.solve_lgs_node(x[ok], u[ok], pair["d"], pair["n"], om0)[0] - truth) / np.linalg.norm(truth)
        got = jr.joint_solve(jr.NODE, x, u, pair["d"], pair["n"], om0, 0.2 * pair["scaling"], jr.PRIORS["free"], valid=ok)
        joint = np.linalg.norm(got["v"] - truth) / np.linalg.norm(truth)
        rows.append((seed, int(ok.sum()), exact, plain, joint, got["flag"], np.abs(got["omega"] - pair["omega"]).max()))
    return rows


def test_rendered_pair_through_the_oracle_chain(pkg):
    """A rendered pair, corners and LK of the C oracle, the sensor omega off by 1e-3 (1, -1, 0.5) rad per frame.
    Recorded with the committed code (seed: tracked points, relative error of v with the exact gyro, plain, joint; error of omega^):
        20: 300   0.0087   0.2737   0.0569   2.5e-4
        21: 299   0.0116   0.2716   0.0766   3.8e-4
        22: 300   0.0165   0.2710   0.1003   4.7e-4
        23: 300   0.0111   0.2730   0.0692   3.3e-4
    The joint error stays above the exact-gyro one: LK's flow error on a rendered pair is not the white noise of the experiment
    above (synth renders the linearised homography), and what of it looks like a rotation goes into omega^.  Asserted: joint < plain / 2."""
    from of_amd import synth
    from of_amd.pipeline import PipelineConfig
    from oracle import image_oracle as io
    for seed, m, exact, plain, joint, flag, dom in rendered(synth, PipelineConfig, io):
        print(f"seed {seed}: {m} points, exact gyro {exact:.4f}, plain {plain:.4f}, joint {joint:.4f}, flag {flag}, omega^ off by {dom:.2e}")
        assert flag == 0
        assert joint < plain / 2, (seed, plain, joint)


# ---------------------------------------------------------------------------------------------------- a prior term that overflows
OVERFLOWING = ((1e-160,) * 3, (1e-160, np.inf, 0.0))             # (d sigma_f)^2 / sigma^2 = 9e-8 / 1e-320 is +inf in f64
FINITE_NEIGHBOUR = (1e-153,) * 3                                 # the prior term is 9e298: finite, and the variance 1e-306 still a normal f64


@pytest.mark.parametrize("variant", (jr.NODE, jr.SIM))
def test_a_prior_term_that_overflows_is_not_attempted(variant):
    """ofk.h: flag 1 where "any joint sum or result is not finite".  joint_finish adds (d sigma_f)^2 / sigma_k^2 to S's diagonal and
    ends, before the eigenvalues are formed, where an entry of S is not finite: flag 1, omega^ = omega0, the kept count and the
    solve's fields before stay, slots 3-5 and 12-26 are 0.  A value just large enough for the term to stay finite is flag 0, delta
    is of the order c / 9e298, and the stacked lstsq agrees (its columns scaled: beside prior rows of 3e149 lstsq's rank cut would
    take v's columns for null)."""
    import warnings
    x, u, d, nrm, om0, v, om = jr.scene(65, 1065)
    vs, rss, rank = jr.plain_solve(variant, x, u, d, nrm, om0)
    for prior in OVERFLOWING:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = jr.joint_solve(variant, x, u, d, nrm, om0, jr.SIGMA_FLOW, prior)
        rec = got["rec"]
        assert got["flag"] == 1 and rec[10] == 1.0 and not got["rewritten"], prior
        assert np.array_equal(got["v"], vs) and got["rss"] == rss and np.array_equal(got["omega"], om0)
        assert np.array_equal(rec[0:3], om0) and np.array_equal(rec[6:9], vs) and rec[9] == rss and rec[11] == 65
        assert not rec[3:6].any() and not rec[12:].any(), rec
    got = jr.joint_solve(variant, x, u, d, nrm, om0, jr.SIGMA_FLOW, FINITE_NEIGHBOUR)
    assert got["flag"] == 0 and got["rewritten"] and np.all(np.isfinite(got["rec"]))
    assert np.all(got["rec"][12:15] > 1e298) and np.abs(got["rec"][3:6]).max() < 1e-290
    vl, ol = jr.joint_lstsq(variant, x, u, d, nrm, om0, jr.SIGMA_FLOW, FINITE_NEIGHBOUR, scale_columns=True)
    assert jr.rel_dev(got["v"], got["omega"], vl, ol) <= TOL
    assert np.linalg.norm(got["v"] - vs) <= 1e-290                # ... which is the plain solve: the prior holds every axis


def test_two_points():
    """Two points: three independent rows for v (rank 3), but S is singular with every axis free - its eigenvalues about 3.8, 1e-15,
    -3e-15: flag 2.  A prior of 1e-3 makes it a problem again."""
    x, u, d, nrm, om0, v, om = jr.scene(8, 6)
    vs, rss, rank = jr.plain_solve(jr.NODE, x[:2], u[:2], d, nrm, om0)
    assert rank == 3
    free = jr.joint_solve(jr.NODE, x[:2], u[:2], d, nrm, om0, jr.SIGMA_FLOW, jr.PRIORS["free"])
    ls = free["rec"][12:15]
    assert free["flag"] == 2 and free["rec"][11] == 2 and not free["rewritten"] and np.array_equal(free["v"], vs), free["rec"]
    assert 3.0 < ls[0] < 5.0 and np.all(np.abs(ls[1:]) < 1e-13) and not free["rec"][3:6].any() and not free["rec"][15:].any()
    prior = jr.joint_solve(jr.NODE, x[:2], u[:2], d, nrm, om0, jr.SIGMA_FLOW, jr.PRIORS["prior"])
    assert prior["flag"] == 0 and prior["rewritten"]
    vl, ol = jr.joint_lstsq(jr.NODE, x[:2], u[:2], d, nrm, om0, jr.SIGMA_FLOW, jr.PRIORS["prior"])
    assert jr.rel_dev(prior["v"], prior["omega"], vl, ol) <= TOL


def sensor_row(d, nrm, omega, scaling=1e-3, cx=640.0, cy=480.0):
    """A sensor row (ofk.h) with the slots the resident references read."""
    sr = np.zeros(32)
    sr[0] = d; sr[1:4] = nrm; sr[4:7] = omega; sr[7:16] = np.eye(3).ravel(); sr[19] = scaling; sr[20] = cx; sr[21] = cy
    return sr


def pixel_points(x, u, sr):
    """f32 pixel tracks whose scaled points are (close to) x, u."""
    nxt = (x / sr[19] + [sr[20], sr[21]]).astype(np.float32)
    prev = (nxt.astype(np.float64) - u / sr[19]).astype(np.float32)
    return prev, nxt


def test_pair_joint_behind_an_unsolved_step():
    """solved=False (a stream step whose record[15] is 0): flag 1 in the header's layout whatever the points are, v / rss the record's
    own - a step that did not solve leaves v = 0, rss = 0, rank 0 - and the same points with solved=True solve."""
    x, u, d, nrm, om0, v, om = jr.scene(65, 1065)
    sr = sensor_row(d, nrm, om0)
    prev, nxt = pixel_points(x, u, sr)
    status = np.ones(65, np.uint8); status[7::9] = 0
    for rec in (np.zeros(16), np.concatenate([[0.01, -0.02, 0.003, 4e-7, 3.0], np.zeros(11)])):
        got = jr.pair_joint(jr.NODE, prev, nxt, status, sr, 0.2, (1e-3,) * 3, rec, solved=False)
        r = got["rec"]
        assert got["flag"] == 1 and r[10] == 1.0 and not got["rewritten"]
        assert np.array_equal(got["v"], rec[0:3]) and got["rss"] == rec[3] and np.array_equal(got["omega"], om0)
        assert np.array_equal(r[0:3], om0) and np.array_equal(r[6:10], rec[0:4]) and r[11] == np.count_nonzero(status)
        assert not r[3:6].any() and not r[12:].any()
    on = jr.pair_joint(jr.NODE, prev, nxt, status, sr, 0.2, (1e-3,) * 3, rec, solved=True)
    assert on["flag"] == 0 and on["rewritten"]
