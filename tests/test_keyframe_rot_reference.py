"""The numpy restatement of the keyframe's rotation refined from the flow (tests/keyframe_rot_reference.py) and its experiments.

Measured with the restatement (hover geometry of keyframe_reference: f = 1000 px, d = 10, 0.2 px of noise on key AND current pixels).
(a) pair(): one pair, keyframe age 30, R_acc off by e ~ N(0, err^2) per axis, the prior matched, rms over seeds 0-11 of |T - truth| / d,
    plain key solve | joint solve (two Gauss-Newton steps, gate 2 px):
      err      200 points                      64 points
      0        5.74e-5 | the same bits (held)  1.57e-4 | the same bits
      5e-5     7.59e-5 | 8.07e-5 (x 1.063)     1.74e-4 | 1.73e-4 (x 0.994)
      2e-4     2.34e-4 | 2.12e-4               3.64e-4 | 3.13e-4
      1e-3     1.17e-3 | 3.00e-4 (3.9)         1.69e-3 | 5.40e-4 (3.1)
      5e-3     5.93e-3 | 3.08e-4 (19.3)        8.53e-3 | 5.58e-4 (15.3)
      2e-2     2.35e-2 | 3.09e-4 (76)          3.38e-2 | 5.57e-4 (61)
    the rotation comes back to 2.8e-4 rad (200 points) / 5.2e-4 rad (64).  Without the gate (whose second solve takes further steps),
    200 points: one step 7.67e-4 at 2e-2 against 3.09e-4 with two (x 2.49); at 5e-3 3.075e-4 against 3.080e-4.
    Inside 3 sigma (Mahalanobis, 3 degrees of freedom) over the 120 trials with err > 0: delta 106 (0.88), T 111 (0.93).
(b) chain(): 200 steps, default re-keying, seeds 0-2, position error / d at step 200, rms, keyframe alone | with the rotation:
      gyro bias 1e-4 per frame, sigma_bias 1e-4:         0.0299  | 1.84e-4 (162)
      white gyro noise 2e-5 per frame, sigma_gyro 2e-5:  3.19e-4 | 1.88e-4 (1.70)
    and at step 100:
      source attitude, exact R_world, gyro bias 1e-4:    0.0151  | 3.057e-5, the error-free gyro chain's 3.058e-5 (ratio 1.00)
      source attitude, R_world off by 1e-3 rad per axis: 2.15e-3 with the prior holding (sigma_att 1e-9) | 2.11e-4 with sigma_att 1e-3 (10.2)
Gains are asserted at half of what was measured: one seed is one draw of the noise."""
import numpy as np
import pytest

import keyframe_reference as kr
import keyframe_rot_reference as RR

rms = lambda v: float(np.sqrt(np.mean(np.square(v))))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_plain(out, rec, want_out, want_rec, tag):
    for k in ("key_xy", "member", "state", "istate"):
        assert np.array_equal(bits(out[k]), bits(want_out[k])), (tag, k)
    assert np.array_equal(bits(rec), bits(want_rec)), (tag, rec, want_rec)


# ------------------------------------------------------------------------------------------------ 1. held axes
@pytest.mark.parametrize("r", [RR.setting(axes=(0, 0, 0)), RR.setting(sigma_gyro=0.0, sigma_bias=0.0), RR.setting(source="attitude", sigma_att=0.0)])
def test_all_axes_held_is_the_plain_step_bit_for_bit(r):
    s = kr.setting(rot_max=0.02)                                 # the wobble exceeds 0.02 rad every few steps: re-keys by angle
    S, seed = 60, 3
    rng = np.random.default_rng(seed)
    Q = np.stack([rng.uniform(-5, 5, S), rng.uniform(-4, 4, S), np.zeros(S)], 1)
    bp, Wp = kr.hover_pose(0, 10.0, seed)
    a, b = kr.empty(S, np.float64), RR.empty(S, np.float64)
    status = np.ones(S, np.uint8)
    for k in range(1, 41):
        bb, W = kr.hover_pose(k, 10.0, seed)
        sn = kr.sensor_row(bb, W, kr.rot_log(W.T @ Wp) + 1e-4)
        obs = kr.project(Q, bb, W)[0] + 0.2 * rng.standard_normal((S, 2))
        a, rec_a, _, _ = kr.step(a, obs, status, S, sn, -(bb - bp), True, k - 1, s, new_count=0, max_total=S)
        b, rec_b, rrec, _, _ = RR.step(b, obs, status, S, sn, -(bb - bp), True, k - 1, s, r, new_count=0, max_total=S)
        same_plain(b, rec_b, a, rec_a, k)
        assert rrec[3] == RR.HELD and not np.delete(rrec, 3).any()
        bp, Wp = bb, W
    assert a["istate"][2] >= 3                                   # re-keys happened


# ------------------------------------------------------------------------------------------------ 2. and 4. the single pair
@pytest.fixture(scope="module")
def sweeps():
    return {n: RR.sweep(npts=n, seeds=12) for n in (200, 64)}


def test_pair_sweep_gains_and_costs(sweeps):
    for n, sw in sweeps.items():
        print(n, {e: (v["plain"], v["joint"], v["delta"]) for e, v in sw.items()})
    # measured gains (docstring): 3.9, 19.3, 76 at 200 points; 3.1, 15.3, 61 at 64: asserted at half
    for n, gains in ((200, {1e-3: 3.9, 5e-3: 19.3, 2e-2: 76.0}), (64, {1e-3: 3.1, 5e-3: 15.3, 2e-2: 61.0})):
        for e, g in gains.items():
            assert sweeps[n][e]["plain"] / sweeps[n][e]["joint"] >= g / 2, (n, e, sweeps[n][e])
    # with no error the matched prior holds every axis: the same solve
    for n in (200, 64):
        assert sweeps[n][0.0]["joint"] == sweeps[n][0.0]["plain"]
    # a small error with its prior: measured 1.063 of the plain solve's error at 200 points (allowed: twice that excess), 0.994 at 64
    assert sweeps[200][5e-5]["joint"] <= (1.0 + 2 * 0.063) * sweeps[200][5e-5]["plain"]
    assert sweeps[64][5e-5]["joint"] <= sweeps[64][5e-5]["plain"]
    # the floor: whatever the gyro did, the joint solve ends at 3.0-3.1e-4 d / 5.4-5.6e-4 d (measured); twice that at most
    for e in (1e-3, 5e-3, 2e-2):
        assert sweeps[200][e]["joint"] <= 2 * 3.1e-4 and sweeps[64][e]["joint"] <= 2 * 5.6e-4


def test_second_gauss_newton_step_matters_at_2e_2_and_not_below_5e_3():
    one = RR.sweep(errs=(5e-3, 2e-2), iters=1, gate=0.0)
    two = RR.sweep(errs=(5e-3, 2e-2), iters=2, gate=0.0)
    print({e: (one[e]["joint"], two[e]["joint"]) for e in one})
    assert one[2e-2]["joint"] >= (1.0 + 1.49 / 2) * two[2e-2]["joint"]       # measured 2.49
    assert abs(one[5e-3]["joint"] / two[5e-3]["joint"] - 1.0) <= 0.02          # measured 0.998


def test_consistency_of_the_covariances(sweeps):
    """The share of trials with delta^ - delta inside 3 sigma of C_delta and T inside 3 sigma of C_T.  Measured 0.88 and 0.93 of 120;
    the floor is 0.75.  The experiment puts 0.2 px on the key AND the current pixels while sigma_flow is 0.2, so the rows are noisier
    than C assumes by sqrt(2); besides, C ignores that the key pixels' noise is shared ACROSS the steps of a keyframe - not within
    one step, which is all this test sees."""
    n_ok = sum(v["n_ok"] for sw in sweeps.values() for e, v in sw.items() if e > 0)
    in_d = sum(v["in3_d"] for sw in sweeps.values() for e, v in sw.items() if e > 0)
    in_T = sum(v["in3_T"] for sw in sweeps.values() for e, v in sw.items() if e > 0)
    print("trials", n_ok, "delta inside 3 sigma", in_d, "T inside 3 sigma", in_T)
    assert n_ok == 120
    assert in_d >= 0.75 * n_ok and in_T >= 0.75 * n_ok


# ------------------------------------------------------------------------------------------------ 3. and 5. the chain
def _chains(r, **kw):
    alone = rms([RR.chain(seed=sd, r=None, **kw)["key"][200] for sd in range(3)])
    rot = rms([RR.chain(seed=sd, r=r, **kw)["key"][200] for sd in range(3)])
    print(kw, "keyframe alone", alone, "with the rotation", rot)
    return alone, rot


def test_readme_case_constant_gyro_error():
    alone, rot = _chains(RR.setting(sigma_bias=1e-4), gyro_bias=1e-4)
    assert abs(alone - 0.030) < 0.001                            # the figure on record
    assert alone / rot >= 162 / 2                                # measured 162


def test_white_gyro_noise():
    alone, rot = _chains(RR.setting(sigma_gyro=2e-5, sigma_bias=0.0), gyro_noise=2e-5)
    assert rot <= 1.25 * alone
    assert alone / rot >= 1.0 + 0.70 / 2                         # a gain shows: measured 1.70


def _chain100(**kw):
    return rms([RR.chain(seed=sd, steps=100, report=(100,), **kw)["key"][100] for sd in range(3)])


def test_source_attitude_exact_reaches_the_error_free_gyro_chain():
    clean = _chain100(r=None)                                    # the error-free gyro chain: 3.058e-5
    att = _chain100(r=RR.setting(source="attitude", sigma_att=1e-6), gyro_bias=1e-4)       # 3.057e-5; the keyframe alone: 0.0151
    print("error-free gyro chain", clean, "attitude source beside a gyro that is off by 1e-4 per frame", att)
    assert att <= 2.0 * clean                                    # measured ratio 1.00


def test_source_attitude_noisy_is_refined():
    held = _chain100(r=RR.setting(source="attitude", sigma_att=1e-9), gyro_bias=1e-4, att_noise=1e-3)
    noisy = _chain100(r=RR.setting(source="attitude", sigma_att=1e-3), gyro_bias=1e-4, att_noise=1e-3)
    print("attitudes off by 1e-3 rad: the prior holding", held, "refined", noisy)
    assert held / noisy >= 10.2 / 2                              # measured 2.15e-3 against 2.11e-4: 10.2


# ------------------------------------------------------------------------------------------------ 6. fallbacks
def _pair_state(S=40, seed=2, err=0.0, clusters=False, noise=0.2):
    rng = np.random.default_rng(seed)
    Q = np.stack([rng.uniform(-5, 5, S), rng.uniform(-4, 4, S), np.zeros(S)], 1)
    if clusters:
        Q = np.array([[-3.0, 2.0, 0.0], [2.5, -1.0, 0.0]])[np.arange(S) % 2]
        noise = 0.0
    b0, W0 = kr.hover_pose(0); b1, W1 = kr.hover_pose(30)
    st = RR.empty(S, np.float64)
    st["key_xy"] = kr.project(Q, b0, W0)[0] + noise * rng.standard_normal((S, 2)); st["member"][:] = 1
    st["state"][:9] = (kr.rotation(np.full(3, err)) @ W1.T @ W0).ravel(); st["istate"] = np.array([0, S, 1, 0], np.int32)
    return st, kr.project(Q, b1, W1)[0] + noise * rng.standard_normal((S, 2)), kr.sensor_row(b1, W1, np.zeros(3))


@pytest.mark.parametrize("case", ["few rows", "coincident", "nan range", "too large", "no keyframe"])
def test_fallbacks_take_their_flag_and_leave_the_plain_result(case):
    s, r = kr.setting(rot_max=3.0), RR.setting(sigma_bias=1e-3)
    st, cur, sn = _pair_state(err=2e-2 if case == "too large" else 1e-3, clusters=case == "coincident")
    S = len(cur)
    status = np.ones(S, np.uint8)
    want_flag, plain_flag = RR.NONE, kr.UNSOLVED
    if case == "few rows":
        status[5:] = 0                                           # five rows: fewer than min_rows
    elif case == "coincident":                                   # two points, twenty times each: T is determined, (T, delta) is not
        r = RR.setting(sigma_bias=np.inf)
        want_flag, plain_flag = RR.SINGULAR, kr.SOLVED
    elif case == "nan range":
        sn[0] = np.nan
    elif case == "too large":
        r = RR.setting(sigma_bias=1e-3, delta_max=5e-3)
        want_flag, plain_flag = RR.LARGE, kr.SOLVED
    else:
        st["istate"][1] = 0
        plain_flag = kr.NONE
    plain = {k: st[k] for k in ("key_xy", "member", "state", "istate")}
    w_out, w_rec, _, _ = kr.step(plain, cur, status, S, sn, np.array([0.01, 0.0, 0.0]), True, 29, s, new_count=0, max_total=S)
    out, rec, rrec, _, _ = RR.step(st, cur, status, S, sn, np.array([0.01, 0.0, 0.0]), True, 29, s, r, new_count=0, max_total=S)
    assert rrec[3] == want_flag and w_rec[3] == plain_flag, (case, rrec[3], w_rec[3])
    same_plain(out, rec, w_out, w_rec, case)
    assert not rrec[13:19].any() and rrec[31] == 0               # no C_delta, no Gauss-Newton step stands
    assert np.array_equal(rrec[4:13], out["state"][:9]) or w_rec[9] != 0     # R^ is R_acc (the state's, unless the step re-keyed)
    if case == "too large":
        assert np.linalg.norm(rrec[0:3]) > 5e-3                  # the refused correction is reported
    else:
        assert not rrec[0:3].any()
    # and the same inputs with a usable setting are refined (the fallback is the setting's, not the data's) where the data allow
    if case in ("coincident", "too large"):
        _, rec2, rrec2, _, _ = RR.step(st, cur, status, S, sn, np.zeros(3), True, 29, s, RR.setting(sigma_bias=1e-3))
        assert rrec2[3] == RR.OK
