"""GPU: ofk_velocity_solve_robust against tests/robust_reference.py - the three systems, point counts around every chunk and launch
boundary up to 4096, masks that leave fewer than 8 points, both losses, K in {0, 1, 16, 64, 256}, 0 / 1 / 5 / 32 rounds, exact data with
and without outliers (flag 2), a rank-deficient problem (flag 3), outlier shares from 0 to 45 % under 0.05 px of flow noise.

Compared at the suite's tolerances (tests/batch_oracle.py): v rtol 1e-9 / atol 1e-13, singular values 1e-9, residual 1e-6; rank, count,
m, hyp, rounds and flag exactly; s and score rtol 1e-9; weights atol 1e-9.  One bound is looser than that list: singular values BELOW the
rank cut (rank-deficient problems only) are rounding noise of the 3x3 eigen-solve, eps * lambda_max on the squared spectrum, so they are
held to 4 sqrt(eps) s_max absolutely, not to 1e-9 relatively; those that count keep 1e-9.  Two legitimate disagreements are handled, not hidden:
(a) a device hyp other than the reference's must score within 1e-12 (relative) of the reference's best, and the comparison continues
from the device's choice; (b) a TUKEY count may differ by the points whose reference |t - 1| < 1e-9.  The inputs are chosen so that the
reference alone shows a best-to-second score gap >= 1e-6 and no such t (asserted per case), and the last test asserts that neither
allowance was used in more than 1 % of the cases."""
import numpy as np
import pytest

import robust_reference as rr
from oracle import estimation_oracle as eo

pytestmark = pytest.mark.gpu

SC = 1.0 / 640.0                                                # scaled units per pixel
USED = dict(cases=0, hyp=0, count=0)


def make_problem(rng, n, share, noise_px=0.05, arbitrary=False):
    """n points under one camera motion; `share` of them move otherwise (a coherent shift of (-7, +5) px, or arbitrary flows)."""
    x = rng.uniform(-0.45, 0.45, (n, 2)) * np.array([1.0, 0.75])
    v = rng.uniform(-0.005, 0.005, 3); om = rng.uniform(-0.004, 0.004, 3)
    d = rng.uniform(0.8, 1.5); nrm = np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), 1.0]); nrm /= np.linalg.norm(nrm)
    u = eo.generate_test_data(x, v, om, d, nrm)
    out = rng.permutation(n)[:int(round(share * n))]
    if arbitrary:
        u[out] += rng.uniform(-20, 20, (len(out), 2)) * SC
    else:
        u[out] += np.array([-7.0, 5.0]) * SC
    u += rng.standard_normal((n, 2)) * noise_px * SC
    return dict(x=x, u=u, v=v, om=om, d=d, nrm=nrm, wgt=rng.uniform(0.5, 2.0, n), t=rng.uniform(-0.1, 0.1, 3))


def run_device(ctx, ofk, variant, probs, valid, setting, with_t=False):
    x = np.stack([p["x"] for p in probs]); u = np.stack([p["u"] for p in probs])
    kw = dict(nrm=np.stack([p["nrm"] for p in probs]), valid=valid)
    if variant == rr.OFMODULE:
        kw["wgt"] = np.stack([p["wgt"] for p in probs])
    else:
        kw["d"] = np.array([p["d"] for p in probs]); kw["omega"] = np.stack([p["om"] for p in probs])
        if with_t:
            kw["t"] = np.stack([p["t"] for p in probs])
    return ctx.velocity_solve_robust(variant, x, u, robust=ofk.robust_setting(**setting), **kw)


def reference(variant, p, valid, setting, b, force_hyp=None):
    return rr.robust_solve(variant, p["x"], p["u"], p["d"], p["nrm"], p["om"], wgt=p["wgt"] if variant == rr.OFMODULE else None,
                           valid=valid, loss=setting["loss"], c=setting["c"], iters=setting["iters"], hypotheses=setting["hypotheses"],
                           seed=setting["seed"], problem=b, force_hyp=force_hyp)


def compare(variant, p, valid, setting, b, out, w, st, tag, with_t=False, conditions=True):
    ref = reference(variant, p, valid, setting, b)
    USED["cases"] += 1
    print(f"{tag}: m {int(st[3])} hyp {int(st[4])} score {st[5]:.6e} s {st[0]:.6e} rounds {int(st[6])} flag {int(st[7])} count {int(st[2])} "
          f"| ref hyp {int(ref['stats'][4])} gap {ref['gap']:.3e} tmin {ref['tmin']:.3e}")
    if conditions and ref["stats"][7] == 0:
        assert ref["gap"] >= 1e-6 and ref["near"] == 0, (tag, "the case does not meet the comparison's conditions", ref["gap"], ref["tmin"])
    if int(st[4]) != int(ref["stats"][4]):                      # allowance (a)
        best = ref["stats"][5]
        assert int(st[4]) >= 0 and abs(st[5] - best) <= 1e-12 * best, (tag, "hyp", st[4], st[5], ref["stats"][4], best)
        USED["hyp"] += 1
        ref = reference(variant, p, valid, setting, b, force_hyp=int(st[4]))
    rs = ref["stats"]
    assert (int(out[4]), int(st[3]), int(st[4]), int(st[6]), int(st[7])) == (ref["rank"], int(rs[3]), int(rs[4]), int(rs[6]), int(rs[7])), (tag, out[4], st, ref["rank"], rs)
    if st[2] != rs[2]:                                          # allowance (b)
        assert setting["loss"] == rr.TUKEY and abs(st[2] - rs[2]) <= ref["near"], (tag, "count", st[2], rs[2], ref["near"])
        USED["count"] += 1
    v = ref["v"] - (np.cross(p["om"], p["t"]) if with_t else 0.0)
    np.testing.assert_allclose(out[0:3], v, rtol=1e-9, atol=1e-13, err_msg=tag)
    k = ref["rank"]                                              # singular values below the rank cut are rounding noise of the 3x3 eigen-solve:
    np.testing.assert_allclose(out[5:5 + k], ref["s"][:k], rtol=1e-9, err_msg=tag)      # eps * lambda_max on the squared spectrum, i.e. up to
    assert np.all(np.abs(out[5 + k:8] - ref["s"][k:]) <= 4 * np.sqrt(rr.EPS) * max(ref["s"][0], 1e-300)), (tag, out[5:8], ref["s"])   # sqrt(eps) * s_max each
    np.testing.assert_allclose(out[3], ref["r"], rtol=1e-6, atol=1e-18, err_msg=tag)
    np.testing.assert_allclose(st[[0, 5]], rs[[0, 5]], rtol=1e-9, atol=0, err_msg=tag)
    np.testing.assert_allclose(st[1], rs[1], rtol=1e-9, atol=1e-9, err_msg=tag)
    np.testing.assert_allclose(w, ref["weights"], rtol=0, atol=1e-9, err_msg=tag)
    return ref


def setting_of(loss, hypotheses, iters, seed=7):
    return dict(loss=loss, c={rr.HUBER: 1.345, rr.TUKEY: 4.685}[loss], iters=iters, hypotheses=hypotheses, seed=seed)


SIZES = (3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 500, 1000, 4096)


@pytest.mark.parametrize("variant", (rr.NODE, rr.SIM, rr.OFMODULE))
def test_sizes_and_shares(gpu_ctx, ofk, variant):
    rng = np.random.default_rng(100 + variant)
    for n in SIZES:
        shares = (0.0, 0.2, 0.45)
        probs = [make_problem(rng, n, sh) for sh in shares]
        for setting in (setting_of(rr.TUKEY, 64, 5, seed=0x1234ABCD5678 + n), setting_of(rr.HUBER, 16, 1, seed=n)):
            out, w, st = run_device(gpu_ctx, ofk, variant, probs, None, setting, with_t=variant == rr.SIM)
            for b, p in enumerate(probs):
                compare(variant, p, None, setting, b, out[b], w[b], st[b], f"variant {variant} n {n} share {shares[b]} loss {setting['loss']}",
                        with_t=variant == rr.SIM)


@pytest.mark.parametrize("loss", (rr.HUBER, rr.TUKEY))
def test_settings_cross(gpu_ctx, ofk, loss):
    rng = np.random.default_rng(200 + loss)
    shares = (0.0, 0.1, 0.3, 0.45)
    probs = [make_problem(rng, 300, sh, arbitrary=k % 2 == 1) for k, sh in enumerate(shares)]
    for K in (0, 1, 16, 64, 256):
        for iters in (0, 1, 5, 32):
            setting = setting_of(loss, K, iters, seed=(K << 40) + iters)
            out, w, st = run_device(gpu_ctx, ofk, rr.NODE, probs, None, setting)
            for b, p in enumerate(probs):
                ref = compare(rr.NODE, p, None, setting, b, out[b], w[b], st[b], f"loss {loss} K {K} iters {iters} share {shares[b]}")
                if iters == 0:                                  # the start itself: all weights 1
                    assert np.array_equal(w[b], np.ones(300)) and st[b, 6] == 0 and ref["stats"][6] == 0


def test_masks_that_leave_few_points(gpu_ctx, ofk):
    rng = np.random.default_rng(300)
    n = 200
    probs = [make_problem(rng, n, 0.2) for _ in range(6)]
    valid = np.zeros((6, n), np.uint8)
    for b, m in enumerate((0, 1, 3, 7, 8, 150)):
        valid[b, rng.permutation(n)[:m]] = 1
    setting = setting_of(rr.TUKEY, 64, 5)
    out, w, st = run_device(gpu_ctx, ofk, rr.NODE, probs, valid, setting)
    for b, p in enumerate(probs):
        compare(rr.NODE, p, valid[b], setting, b, out[b], w[b], st[b], f"mask leaves {int(valid[b].sum())}", conditions=valid[b].sum() > 8)
        assert np.array_equal(w[b] > 0, valid[b] > 0) or valid[b].sum() >= 8
        if valid[b].sum() < 8:
            assert st[b, 7] == 1 and np.array_equal(w[b], valid[b].astype(np.float64))
    plain = gpu_ctx.velocity_solve(rr.NODE, np.stack([p["x"] for p in probs]), np.stack([p["u"] for p in probs]), d=np.array([p["d"] for p in probs]),
                                   nrm=np.stack([p["nrm"] for p in probs]), omega=np.stack([p["om"] for p in probs]), valid=valid)
    for b in range(4):                                           # fewer than 8 points: today's plain result, bit for bit
        assert np.array_equal(out[b].view(np.uint64), plain[b].view(np.uint64)), b


@pytest.mark.parametrize("loss", (rr.HUBER, rr.TUKEY))
def test_exact_data_stops_with_flag_2(gpu_ctx, ofk, loss):
    rng = np.random.default_rng(400 + loss)
    for variant in (rr.NODE, rr.SIM):
        for n in (8, 65, 500):
            for share, K in ((0.0, 0), (0.0, 64), (0.25, 64), (0.45, 256)):
                probs = [make_problem(rng, n, share, noise_px=0.0, arbitrary=True) for _ in range(3)]
                setting = setting_of(loss, K, 5, seed=n)
                out, w, st = run_device(gpu_ctx, ofk, variant, probs, None, setting)
                for b, p in enumerate(probs):
                    ref = reference(variant, p, None, setting, b)
                    tag = f"exact variant {variant} n {n} share {share} K {K} problem {b}"
                    print(tag, "device", st[b], "err", np.abs(out[b, :3] - p["v"]).max(), "| reference flag", ref["stats"][7], "err", np.abs(ref["v"] - p["v"]).max())
                    if ref["stats"][7] != 2:                     # no all-inlier pair among the samples of this tiny problem: not this test's case
                        assert n == 8 and share > 0, tag
                        continue
                    assert st[b, 7] == 2 and st[b, 6] == 0 and st[b, 3] == n, (tag, st[b])
                    np.testing.assert_allclose(out[b, :3], p["v"], rtol=1e-9, atol=1e-12, err_msg=tag)
                    assert np.array_equal(w[b], np.ones(n)), tag


def test_rank_deficient_problem_keeps_the_plain_start(gpu_ctx, ofk):
    rng = np.random.default_rng(500)
    n = 40
    p = make_problem(rng, n, 0.0)
    p["x"][:] = p["x"][0]                                        # every point at one position: [p]x has rank 2
    setting = setting_of(rr.TUKEY, 64, 5)
    out, w, st = run_device(gpu_ctx, ofk, rr.NODE, [p], None, setting)
    compare(rr.NODE, p, None, setting, 0, out[0], w[0], st[0], "rank deficient", conditions=False)
    assert out[0, 4] == 2 and st[0, 4] == -1 and st[0, 6] == 0 and st[0, 7] == 3 and np.array_equal(w[0], np.ones(n))
    plain = gpu_ctx.velocity_solve(rr.NODE, p["x"], p["u"], d=p["d"], nrm=p["nrm"], omega=p["om"])
    assert np.array_equal(out[0, :3].view(np.uint64), plain[:3].view(np.uint64))


def test_invalid_settings_are_refused(gpu_ctx, ofk):
    rng = np.random.default_rng(600)
    p = make_problem(rng, 50, 0.1)
    for bad in (dict(loss=3), dict(loss=0), dict(c=0.0), dict(c=float("nan")), dict(c=float("inf")), dict(iters=-1), dict(iters=33),
                dict(hypotheses=-1), dict(hypotheses=257)):
        s = dict(setting_of(rr.TUKEY, 16, 2)); s.update(bad)
        with pytest.raises(ofk.OfkError):
            run_device(gpu_ctx, ofk, rr.NODE, [p], None, s)


def test_the_allowances_stayed_rare():
    """Over whatever part of this module ran in this process (all of it in a full run: 401 cases)."""
    print("cases", USED)
    assert USED["hyp"] <= 0.01 * USED["cases"] and USED["count"] <= 0.01 * USED["cases"], USED


def test_python_layers_solve_robustly(pkg, ofk):
    """velocity_node.solve_lgs_robust / simulation.solve_lgs_robust: the reference-shaped wrappers hand their settings through."""
    from of_amd import velocity_node as vn, simulation as sim
    rng = np.random.default_rng(700)
    p = make_problem(rng, 200, 0.3)
    s = setting_of(rr.HUBER, 16, 3, seed=5)
    ref = reference(rr.NODE, p, None, s, 0)
    v, R, rank, sv, w, st = vn.solve_lgs_robust(p["x"], p["u"], p["d"], p["nrm"], p["om"], loss="huber", hypotheses=16, iters=3, seed=5)
    np.testing.assert_allclose(v, ref["v"], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(w, ref["weights"], atol=1e-9)
    assert rank == 3 and R.shape == (1,) and np.array_equal(st[[3, 4, 6, 7]], ref["stats"][[3, 4, 6, 7]])
    s = setting_of(rr.TUKEY, 64, 5, seed=0)
    ref = reference(rr.SIM, p, None, s, 0)
    v, R, sv, w, st = sim.solve_lgs_robust(p["x"], p["u"], p["d"], p["nrm"], p["om"], p["t"])          # the defaults: tukey, 4.685, 5, 64, 0
    np.testing.assert_allclose(v, ref["v"] - np.cross(p["om"], p["t"]), rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(w, ref["weights"], atol=1e-9)
    v, R, rank, sv, w, st = vn.solve_lgs_robust(np.zeros((0, 2)), np.zeros((0, 2)), 1.0, p["nrm"], p["om"])     # no points: zeros, as solve_lgs
    assert not v.any() and rank == 0 and R.size == 0 and w.size == 0 and st[7] == 1
