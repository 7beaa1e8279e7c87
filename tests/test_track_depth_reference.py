"""CPU: the experiment behind the depth per track (tests/track_depth_reference.py; DESIGN.md "Depth per track") - 300 points over the
canopy, 40 steps of constant (v, omega), 0.2 px of flow noise at f = 1000, the per-step v from the epipolar solve's restatement.
The conditions are orderings, not tuned numbers:
  filter against single frame   from step 10 on the median relative depth error of the rows with >= 10 measurements (the state the step
                                starts from, against the truth) is below the same rows' single-frame error |kappa - rho| / rho
  calibration                   |rho^ - rho| <= 3 sqrt(var) on at least 95 % of the mature rows after every step
  map solve                     v_map's relative error is below the plain solve's on every step that has one, and its median within
                                FACTOR of the epipolar v's median
  range reading wrong           d0 off by +20 % from step 20 on, update = 0 from there: the epipolar v is off by 20 %, v_map stays at its
                                earlier noise level plus what predicting with the wrong v_z can add, a tenth of the epipolar v's error at most
Recorded, not asserted (README.md): the two depth errors at steps 5 / 10 / 20 / 40 and v_map's error; printed with -s."""
import functools

import numpy as np
import pytest

import epi_reference as er
import track_depth_reference as T

SEEDS = (1, 2, 3)
# v_map solves three unknowns from every mature row with the depths known to a quarter of a percent, the epipolar solve a direction
# from all rows and the scale from the ten anchor points of one frame: v_map should not be the worse one.  A factor of 2 allows for the
# depths' common error, which they inherit from the scales of the frames that made them.  Measured: 0.46 .. 0.63.
FACTOR = 2.0


@functools.lru_cache(maxsize=None)
def run(seed, wrong=False):
    return T.experiment(seed, d_wrong_from=20, freeze_from=20) if wrong else T.experiment(seed)


def mature_after(r, s=T.DEFAULTS):
    return (r["nobs_post"] >= s["min_obs"]) & (r["rho_post"] > 0) & (r["var_post"] <= (s["rel_max"] * r["rho_post"]) ** 2)


def depth_errors(r, nobs_min=10):
    m = r["nobs_prior"] >= nobs_min
    filt = np.abs(r["rho_prior"] - r["rho_true"])[m] / r["rho_true"][m]
    single = np.abs(r["z"] - r["rho_true"])[m] / r["rho_true"][m]
    return int(m.sum()), float(np.median(filt)) if m.any() else np.nan, float(np.median(single)) if m.any() else np.nan


@pytest.mark.parametrize("seed", SEEDS)
def test_filter_beats_the_single_frame(seed):
    out = run(seed)
    for t in range(10, T.STEPS):
        n, filt, single = depth_errors(out[t])
        assert n >= 50 and filt < single, (t, n, filt, single)
    print("seed", seed, "median relative depth error (filtered, single frame) behind steps 5 / 10 / 20 / 40:",
          [tuple(round(e, 5) for e in depth_errors(out[t - 1], min(10, t - 1))[1:]) for t in (5, 10, 20, 40)])       # the rows as old as the run allows


@pytest.mark.parametrize("seed", SEEDS)
def test_variance_is_calibrated(seed):
    shares = []
    for t, r in enumerate(run(seed)):
        m = mature_after(r)
        if t >= 3:
            assert m.sum() >= 100, (t, int(m.sum()))             # every step keeps mature rows
        if m.any():
            shares.append(float((np.abs(r["rho_post"] - r["rho_next"])[m] <= 3.0 * np.sqrt(r["var_post"][m])).mean()))
    assert min(shares) >= 0.95, shares
    print("seed", seed, "smallest share inside 3 sigma:", round(min(shares), 4))


@pytest.mark.parametrize("seed", SEEDS)
def test_map_solve_against_the_other_solves(seed):
    out = run(seed)
    assert [r["flag"] for r in out[:3]] == [1, 1, 1] and not any(r["flag"] for r in out[3:])       # min_obs = 3 measurements first
    assert not any(r["epi_flag"] for r in out)
    vm = np.array([T.rel_err(r["v_map"]) for r in out]); ep = np.array([T.rel_err(r["v_epi"]) for r in out])
    pl = np.array([T.rel_err(r["v_plain"]) for r in out])
    assert np.all(vm[3:] < pl[3:]), (vm, pl)
    ratio = np.median(vm[10:]) / np.median(ep[10:])
    assert ratio <= FACTOR, ratio
    print("seed", seed, "median relative error from step 10 on: v_map", round(float(np.median(vm[10:])), 5), "epipolar", round(float(np.median(ep[10:])), 5),
          "plain", round(float(np.median(pl[10:])), 4), "ratio", round(float(ratio), 3))


@pytest.mark.parametrize("seed", SEEDS)
def test_map_solve_outlives_a_wrong_range_reading(seed):
    out = run(seed, wrong=True)
    vm = np.array([T.rel_err(r["v_map"]) for r in out]); ep = np.array([T.rel_err(r["v_epi"]) for r in out])
    # "Its earlier error" is a noise level, not a number: the ten steps before the reading goes wrong sample it (rms), a later step
    # may draw 3 of them (the norm of three Gaussian components passes 3 rms less than once in 10^4), and the noise grows as the
    # mature rows leave the frame, with the root of their number.  On top of it comes the drift the test is after: the frozen depths
    # are still predicted with the step's v, whose v_z is 20 % long, so rho moves by at most 0.2 v_z rho per step.
    noise, rows = np.sqrt(np.mean(vm[10:20] ** 2)), np.mean([r["mature"] for r in out[10:20]])
    rho_max = 1.0 / (er.D * 0.5)                                 # the canopy reaches half the height
    for t in range(20, T.STEPS):
        assert out[t]["flag"] == 0 and out[t]["mature"] >= T.DEFAULTS["min_rows"], t
        assert 0.15 < ep[t] < 0.25, (t, ep[t])                   # the scale follows the reading
        assert vm[t] <= 3.0 * noise * np.sqrt(rows / out[t]["mature"]) + (t - 19) * 0.2 * abs(er.V[2]) * rho_max, (t, vm[t], noise)
        assert vm[t] < ep[t] / 10.0, (t, vm[t], ep[t])
    fresh = run(seed)
    assert all(np.array_equal(a["v_map"], b["v_map"]) for a, b in zip(out[:20], fresh[:20]))
    print("seed", seed, "v_map's error at steps 20 / 30 / 40 under the wrong reading:", [round(float(vm[t - 1]), 4) for t in (20, 30, 40)],
          "epipolar:", [round(float(ep[t - 1]), 3) for t in (20, 30, 40)], "mature rows:", [out[t - 1]["mature"] for t in (20, 30, 40)])


def test_restatement_paths():
    """step() on its own edges: every skip and reset path, update = 0, gate = 0, an unsolved step, appended rows and their clamp."""
    s = T.setting(sigma_flow=2e-4, b_min=0.5e-3)
    x, u, d, nrm, om, v, rho = er.scene(40, 7)
    st = T.empty(48)
    st, rec, count, _ = T.step(st, x, u, np.ones(40), 40, om, v, True, s, new_count=20, max_total=44)
    assert count == 44 and rec[6] == 40 and rec[3] == 1 and np.all(st["nobs"][:40] == 1) and not st["nobs"][40:].any()
    x2 = np.concatenate([x, np.zeros((8, 2))]); u2 = np.concatenate([u, np.zeros((8, 2))])
    u2[0] += 50 * 2e-4                                           # across and along the epipolar line: one of the two gates takes it
    x2[1] = np.nan                                               # no measurement, and no prediction either: the row is reset
    x2[2] = v[:2] / v[2]                                         # the focus of expansion: |b| = 0
    keep = np.ones(48); keep[5] = 0
    st2, rec2, count2, dg = T.step(st, x2, u2, keep, 44, om, v, True, s)
    assert count2 == 43 and rec2[5] + rec2[7] + rec2[8] + rec2[9] + rec2[6] <= 43 and rec2[7] >= 2 and rec2[8] + rec2[9] >= 1 and rec2[20] >= 1
    st3, rec3, _, _ = T.step(st, x2, u2, keep, 44, om, v, True, dict(s, update=0))
    assert rec3[5] == 0 and np.array_equal(st3["nobs"][:43] <= 1, np.ones(43, bool))
    st4, rec4, _, _ = T.step(st, x2, u2, keep, 44, om, v, True, dict(s, gate=0.0))
    assert rec4[8] == 0 and rec4[9] == 0 and rec4[5] >= rec2[5]
    st5, rec5, _, _ = T.step(st, x2, u2, keep, 44, om, v, False, dict(s, q=1e-6))
    assert rec5[5:10].sum() == 0 and rec5[19] == 0 and np.array_equal(st5["rho"][:4], st["rho"][:4]) and np.allclose(st5["var"][:4], st["var"][:4] + 1e-6)
