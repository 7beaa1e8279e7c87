"""CPU-only: a stream's gyro bias of ofk.h (ofk_set_gyro_bias) as tests/bias_reference.py restates it - against the batch information
fusion it must equal without process noise, at its held axes and flags, and on the experiment that motivates it.

TOL_BIAS, the tolerance the GPU tests hold the device to as well, is pinned here: 16 x the largest relative deviation of (b^, P)
between the sequential filter (q = 0, T = 6 steps) and the batch fusion (P0^-1 + sum R_k^-1)^-1 (P0^-1 b0 + sum R_k^-1 (omega_gyro,k -
omega^_k)) over joint_reference.COUNTS and the three held / free patterns.  The model is linear in omega, so omega^_k does not depend
on the b^ it was linearised at: the batch route takes omega^_k from joint solves at the RAW gyro, the filter from solves at omega - b^.
The sweep runs over the three patterns at p0 = 1e-2 (NODE) and over free / mixed at the prior scales 1e-4 ... 1e8 (NODE and SIM).
Measured: 2.98e-14 (1025 points, SIM, over the prior scales; 2.08e-14 over the three patterns at p0 = 1e-2), with P_EE := R (S^-1 P)_EE.
With P := P - (K S) K^T, the first form, it was 7.04e-12 at p0 = 1e-2 and grew with the prior: 8.4e-8 at 1, 3.3e-4 at 1e2, and from
1e4 on P turned indefinite.

The experiment (experiment(): 40 steps; 200 or 64 points over 1280 x 960 at f = 1000; d = 1.5; v and omega new at every step; a gyro
bias of (3, -3, 1.5)e-3 per frame, 2e-5 of white gyro noise, 0.2 px of flow noise; the filter with p0 = 1e-2, q = 1e-12, every axis
free), mean relative error of v over steps 20-39, six seeds, measured with the committed code:
    points   raw gyro      per-frame joint   gyro less the filtered bias   ratio to joint   ratio to raw     worst |b^ - b| / sqrt(tr P)
    200      0.277-0.296   0.0065-0.0103     0.0029-0.0043                 0.31-0.46        0.0104-0.0149    2.49
    64       0.272-0.301   0.0155-0.0202     0.0043-0.0055                 0.26-0.29        0.0153-0.0183    1.70
After the first step the corrected plain solve is at 0.003-0.011 (200 points) and 0.007-0.022 (64 points)."""
import numpy as np
import pytest

import bias_reference as br
import joint_reference as jr
from oracle import estimation_oracle as eo

TOL_BIAS = 16 * 2.98e-14                                        # 16 x the measured 2.98e-14, see above
MEASURED = dict(dev=0.0)
PATTERNS = {"free": (1e-2, 1e-2, 1e-2), "mixed": (0.0, 1e-2, 5e-3), "held": (0.0, 0.0, 0.0)}
B0 = np.array([1e-3, -2e-3, 5e-4])
BIAS = 1e-3 * np.array([3.0, -3.0, 1.5])
SIGMA_GYRO = 2e-5


def scaled_p0(pattern, scale):
    """The pattern's p0 with its largest value at `scale` (PATTERNS' own: 1e-2)."""
    return tuple(np.asarray(PATTERNS[pattern]) * (scale / 1e-2))


def assert_psd(P, tag):
    """Every eigenvalue of P at or above -4 eps x the largest: what rounding alone may leave of a positive semi-definite matrix."""
    lam = np.linalg.eigvalsh(np.asarray(P, np.float64))
    assert np.all(np.isfinite(lam)) and lam[0] >= -4 * jr.EPS * lam[-1], (tag, lam)


def fusion_deviation(n, pattern, scale=1e-2, variant=jr.NODE, each=None):
    """each: called with (step, record) behind every filter step."""
    s = br.setting(sigma_flow=jr.SIGMA_FLOW, sigma_gyro=SIGMA_GYRO, q=0.0, p0=scaled_p0(pattern, scale), b0=B0)
    free = np.where(s["p0"] > 0, np.inf, 0.0)
    st = br.initial_state(s)
    raws, hats, Rs = [], [], []
    for k in range(6):
        x, u, d, nrm, om0, v, om = jr.scene(n, 2000 + 10 * n + k)
        raw = np.where(s["p0"] > 0, om + BIAS, om + s["b0"])      # a held axis is held at the truth: b0 there is the bias
        st, j = br.step(s, st, variant, x, u, d, nrm, raw)
        assert st[18] == (0.0 if pattern != "held" else 4.0), (n, pattern, scale, k, st[18])
        if each is not None:
            each(k, st)
        lin = np.where(s["p0"] > 0, raw, raw - s["b0"])           # linearised at the raw gyro on every estimated axis
        j0 = jr.joint_solve(variant, x, u, d, nrm, lin, jr.SIGMA_FLOW, free)
        raws.append(raw); hats.append(j0["omega"]); Rs.append(jr.untri(j0["rec"][15:21]) + SIGMA_GYRO ** 2 * np.eye(3))
    b, P = br.batch_fusion(s, raws, hats, Rs)
    return st, br.rel_dev(st[0:3], jr.untri(st[3:9]), b, P)


@pytest.mark.parametrize("n", jr.COUNTS)
def test_sequential_filter_is_the_batch_fusion(n):
    for pattern in PATTERNS:
        st, dev = fusion_deviation(n, pattern)
        MEASURED["dev"] = max(MEASURED["dev"], dev)
        assert dev <= TOL_BIAS, (n, pattern, dev)
        assert st[21] == 6 and st[20] == (0 if pattern == "held" else 6)
    print(f"n {n}: largest relative deviation of (b^, P) so far {MEASURED['dev']:.3e}")


PRIOR_SCALES = (1e-4, 1e-2, 1.0, 1e2, 1e4, 1e8)


@pytest.mark.parametrize("n", jr.COUNTS)
def test_sequential_filter_is_the_batch_fusion_at_every_prior_scale(n):
    """p0 = 1e8 is "I do not know the bias": P0 = 1e16 against an R of 1e-10 and below.  P - (K S) K^T, the form this filter had first,
    cancels there: 7.0e-12 at p0 = 1e-2, 8.4e-8 at 1, 3.3e-4 at 1e2, and at 1e4 with 1025 points P is indefinite after the first update
    and the stream stays in flag 2.  R S^-1 P stays at 2.5e-14 and below over the whole sweep."""
    worst = 0.0
    for scale in PRIOR_SCALES:
        for pattern in ("free", "mixed"):
            for variant in (jr.NODE, jr.SIM):
                tag = (n, scale, pattern, variant)

                def each(k, st):
                    P = jr.untri(st[3:9])
                    assert st[18] == 0 and st[20] == k + 1 and st[21] == k + 1, (tag, k, st[18:22])
                    assert_psd(P, (tag, k))
                    if pattern == "mixed":
                        assert st[0] == B0[0] and not P[0].any() and not P[:, 0].any(), (tag, k, st[0:9])
                st, dev = fusion_deviation(n, pattern, scale, variant, each)
                worst = max(worst, dev)
                MEASURED["dev"] = max(MEASURED["dev"], dev)
                assert dev <= TOL_BIAS, (tag, dev)
    print(f"n {n}: largest relative deviation of (b^, P) over the prior scales {worst:.3e}, so far {MEASURED['dev']:.3e}")


def test_held_axes_keep_b0_and_zero_rows_of_P():
    st, _ = fusion_deviation(65, "mixed")
    P = jr.untri(st[3:9])
    assert st[0] == B0[0] and np.all(P[0] == 0) and np.all(P[:, 0] == 0)
    assert st[1] != B0[1] and st[2] != B0[2] and 0 < P[1, 1] < 1e-4 and 0 < P[2, 2] < 2.5e-5
    assert abs(st[1] - BIAS[1]) < 1e-4 and abs(st[2] - BIAS[2]) < 1e-4
    st, _ = fusion_deviation(65, "held")
    assert np.array_equal(st[0:3], B0) and np.all(st[3:9] == 0) and st[18] == 4.0 and np.all(st[15:18] == 0)


def test_flags_leave_the_bias_alone_and_still_predict():
    s = br.setting(sigma_flow=jr.SIGMA_FLOW, sigma_gyro=SIGMA_GYRO, q=1e-8, p0=(1e-2, 0.0, 1e-2), b0=B0)
    st0 = br.initial_state(s)
    x, u, d, nrm, om0, v, om = jr.scene(65, 11)
    raw = om + BIAS
    predicted = st0[3:9] + np.array([1e-8, 0, 0, 0, 0, 1e-8])
    # flag 1: a non-finite range, the solve does not solve
    st, j = br.step(s, st0, jr.NODE, x, u, np.nan, nrm, raw)
    assert st[18] == 1.0 and np.array_equal(st[0:3], B0) and np.array_equal(st[3:9], predicted) and st[20] == 0 and st[21] == 1
    assert np.array_equal(st[12:15], raw - B0)
    # flag 2: collinear points leave the rotation about their line unobservable
    xc = np.stack([np.linspace(-0.5, 0.5, 20), np.zeros(20)], 1)
    uc = eo.generate_test_data(xc, v, om, d, nrm)
    st, j = br.step(s, st0, jr.NODE, xc, uc, d, nrm, raw, v_s=v, rss_s=0.0, rank=3)
    assert st[18] == 2.0 and np.array_equal(st[0:3], B0) and np.array_equal(st[3:9], predicted) and st[20] == 0
    # flag 3: the gate
    gated = dict(s, nis_max=1e-3)
    st, j = br.step(gated, st0, jr.NODE, x, u, d, nrm, raw)
    assert st[18] == 3.0 and st[19] > 1e-3 and np.array_equal(st[0:3], B0) and np.array_equal(st[3:9], predicted) and st[20] == 0
    assert np.all(st[22:28][[0, 3, 5]] >= 0) and st[28] == 65
    # ... and the same step passes an open gate
    st, j = br.step(s, st0, jr.NODE, x, u, d, nrm, raw)
    assert st[18] == 0.0 and st[20] == 1 and st[1] == B0[1] and abs(st[0] - BIAS[0]) < 2e-4
    # update off: apply only
    st, j = br.step(dict(s, update=False), st0, jr.NODE, x, u, d, nrm, raw)
    assert st[18] == 4.0 and np.array_equal(st[0:9], st0[0:9]) and st[21] == 1


def experiment(seed, n, steps=40, p0=1e-2, each=None):
    """Relative errors of v per step: plain at the raw gyro, per-frame joint, plain at the gyro less the filtered bias; and the worst
    |b^ - b| / sqrt(tr P).  each: called with (step, record) behind every filter step."""
    rng = np.random.default_rng(seed)
    s = br.setting(sigma_flow=jr.SIGMA_FLOW, sigma_gyro=SIGMA_GYRO, q=1e-12, p0=p0)
    st = br.initial_state(s)
    nrm = np.array([0.05, -0.08, 1.0]); nrm /= np.linalg.norm(nrm)
    d = 1.5
    err = np.zeros((steps, 3)); worst = 0.0
    for k in range(steps):
        x = rng.uniform(-1.0, 1.0, (n, 2)) * [0.64, 0.48]
        v = np.array([0.02, -0.015, 0.004]) * rng.uniform(0.5, 1.5, 3); om = np.array([0.004, -0.003, 0.01]) * rng.uniform(-1.5, 1.5, 3)
        u = eo.generate_test_data(x, v, om, d, nrm) + rng.normal(0, jr.SIGMA_FLOW, (n, 2))
        raw = om + BIAS + rng.normal(0, SIGMA_GYRO, 3)
        nv = np.linalg.norm(v)
        err[k, 0] = np.linalg.norm(jr.plain_solve(jr.NODE, x, u, d, nrm, raw)[0] - v) / nv
        err[k, 1] = np.linalg.norm(jr.joint_solve(jr.NODE, x, u, d, nrm, raw, jr.SIGMA_FLOW, (np.inf,) * 3)["v"] - v) / nv
        used = raw - st[0:3]
        err[k, 2] = np.linalg.norm(jr.plain_solve(jr.NODE, x, u, d, nrm, used)[0] - v) / nv
        st, j = br.step(s, st, jr.NODE, x, u, d, nrm, raw)
        assert st[18] == 0.0
        if each is not None:
            each(k, st)
        worst = max(worst, np.linalg.norm(st[0:3] - BIAS) / np.sqrt(st[3] + st[6] + st[8]))
    return err, worst


@pytest.mark.parametrize("n", (200, 64))
def test_filtered_bias_beats_the_per_frame_joint_solve(n):
    rows = []
    for seed in range(6):
        err, worst = experiment(100 + seed, n)
        raw, joint, filt = err[20:].mean(0)
        rows.append((raw, joint, filt, filt / joint, filt / raw, worst, err[1, 2]))
        print(f"n {n} seed {seed}: raw {raw:.4f} joint {joint:.4f} filtered {filt:.4f} ratio to joint {filt / joint:.3f} to raw {filt / raw:.4f} "
              f"worst |b^-b|/sqrt(tr P) {worst:.2f} step 1 {err[1, 2]:.4f}")
    for raw, joint, filt, rj, rr, worst, first in rows:
        assert filt <= 0.6 * joint, (n, filt, joint)
        assert filt <= 0.05 * raw, (n, filt, raw)
        assert worst <= 4.0, (n, worst)


@pytest.mark.parametrize("n", (200, 64))
def test_a_wide_prior_stays_consistent_over_forty_steps(n):
    """p0 = 1e2 with process noise: P falls from 1e4 to 1e-10 at the first update and is predicted and updated 39 times more."""
    def each(k, st):
        assert st[18] == 0 and st[20] == k + 1, (n, k, st[18:22])
        assert_psd(jr.untri(st[3:9]), (n, k))
    for seed in range(2):
        err, worst = experiment(100 + seed, n, p0=1e2, each=each)
        print(f"n {n} seed {seed}: worst |b^-b|/sqrt(tr P) {worst:.2f}")
        assert worst <= 4.0, (n, seed, worst)


def collinear():
    """20 points on one line, the flow of jr.scene's motion: the plain solve reaches rank 3, the rotation about the line is not seen."""
    x, u, d, nrm, om0, v, om = jr.scene(65, 11)
    xc = np.stack([np.linspace(-0.5, 0.5, 20), np.zeros(20)], 1)
    return xc, eo.generate_test_data(xc, v, om, d, nrm), d, nrm, om


def degenerate_cases():
    """The steps that must not update, by name: (keywords of bias_reference.step's problem, state override or None, flag, kept points).
    tests/test_gpu_bias_edges.py holds the device to these flags, so they are asserted here first."""
    x, u, d, nrm, om0, v, om = jr.scene(65, 11)
    raw = om + BIAS
    xc, uc, dc, nrmc, omc = collinear()
    base = dict(x=x, u=u, d=d, nrm=nrm, raw=raw, valid=None)
    cases = {"negative P": (base, dict(P=-np.array([1.0, 0, 0, 1.0, 0, 1.0])), 2, 65),
             "NaN omega": (dict(base, raw=raw * [1, np.nan, 1]), None, 1, 65),
             "inf omega": (dict(base, raw=raw + [0, 0, np.inf]), None, 1, 65),
             "NaN bias": (base, dict(b=B0 * [np.nan, 1, 1]), 1, 65),
             "one point": (dict(base, x=x[:1], u=u[:1]), None, 1, 1),
             "two points": (dict(base, x=x[:2], u=u[:2]), None, 2, 2),           # rank 3 for v: the core runs, 4 rows for 5 unknowns
             "two equal points": (dict(base, x=x[[0, 0]], u=u[[0, 0]]), None, 1, 2),
             "no valid point": (dict(base, valid=np.zeros(65, np.uint8)), None, 1, 0),
             "collinear": (dict(base, x=xc, u=uc, raw=omc + BIAS), None, 2, 20)}
    return cases


def degenerate_state(s, override):
    st = br.initial_state(s)
    if override and "P" in override:
        st[3:9] = override["P"]
    if override and "b" in override:
        st[0:3] = override["b"]
    return st


DEGENERATE_SETTING = dict(sigma_flow=jr.SIGMA_FLOW, sigma_gyro=SIGMA_GYRO, q=1e-8, p0=(1e-2, 0.0, 1e-2), b0=B0)


@pytest.mark.parametrize("name", ("negative P", "NaN omega", "inf omega", "NaN bias", "one point", "two points", "two equal points", "no valid point",
                                  "collinear"))
def test_degenerate_steps_flag_and_leave_the_prediction(name):
    s = br.setting(**DEGENERATE_SETTING)
    prob, override, flag, kept = degenerate_cases()[name]
    st0 = degenerate_state(s, override)
    predicted = st0[3:9] + np.array([1e-8, 0, 0, 0, 0, 1e-8])
    if name in ("collinear", "two points"):                      # the solve itself solves: flag 2 is the core's, not "not attempted"
        assert jr.plain_solve(jr.NODE, prob["x"], prob["u"], prob["d"], prob["nrm"], prob["raw"] - st0[0:3])[2] == 3
    st, j = br.step(s, st0, jr.NODE, prob["x"], prob["u"], prob["d"], prob["nrm"], prob["raw"], valid=prob["valid"])
    assert st[18] == flag, (name, st[18])
    assert np.array_equal(bits64(st[0:3]), bits64(st0[0:3])) and np.array_equal(st[3:9], predicted), (name, st[0:9])
    assert st[20] == 0 and st[21] == 1 and st[28] == kept, (name, st[20], st[21], st[28])
    assert not st[15:18].any() and st[19] == 0 and not st[22:28].any()
    assert np.array_equal(bits64(st[9:12]), bits64(np.asarray(prob["raw"], np.float64)))
    if name in ("NaN omega", "inf omega", "NaN bias"):
        assert not np.all(np.isfinite(st[12:15])), (name, st[12:15])


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
