"""GPU: a stream's gyro bias (ofk_set_gyro_bias / ofk_gyro_bias_step) away from the one operating point of tests/test_gpu_bias.py:
priors from 1e-4 to 1e8, steps that do not update, batches past one 64-thread block of k_gyro_bias_apply, stream steps that do not
solve, streams without tracks, hold_on_skip, the settings the bias had not met, and the facades.

The references and tolerances are those of tests/test_gpu_bias.py (assert_bias_close at TOL_BIAS, REC_TOL for delta, NIS and R) and the
flags are asserted on tests/bias_reference.py first (tests/test_bias_reference.py states them on the CPU), so no case asks the device
which way a step falls.  What a flagged step leaves is compared to the bit: b^, the predicted P, the zeros, the counters.  Every
"carries the bits of" compares two device runs.  No tolerance is introduced here.
Not here: a stream step that ends early behind the apply launch (the bias_restore destructor of ofk_stream_step).  Every refusal made
on the host stands in front of that launch; what can fail behind it are allocations and device calls, which no test provokes."""
import numpy as np
import pytest

import bias_reference as br
import joint_reference as jr
import second_stage_runs as ssr
from point_stage_helpers import bits
from test_bias_reference import (B0, BIAS, DEGENERATE_SETTING, PRIOR_SCALES, SIGMA_GYRO, TOL_BIAS, assert_psd, collinear, degenerate_cases,
                                 degenerate_state, scaled_p0)
from test_gpu_bias import SEEN, assert_bias_close, assert_twin, bias_keywords, run, setting_of, twin

pytestmark = pytest.mark.gpu


def same(a, b):
    return np.array_equal(bits(np.ascontiguousarray(a, np.float64)), bits(np.ascontiguousarray(b, np.float64)))


# ---------------------------------------------------------------------------------------------------- the stage entry: priors
def prior_scenes(n, k):
    sc = [jr.scene(n, 2000 + 10 * n + k + 100 * b) for b in range(3)]
    return tuple(np.stack([s[i] for s in sc]) for i in range(7))


@pytest.mark.parametrize("variant", (jr.NODE, jr.SIM))
@pytest.mark.parametrize("n", (8, 65, 1025))
def test_stage_entry_at_every_prior_scale(gpu_ctx, ofk, n, variant):
    worst = 0.0
    scenes = [prior_scenes(n, k) for k in range(6)]
    for scale in PRIOR_SCALES:
        for pattern in ("free", "mixed"):
            s = br.setting(sigma_flow=jr.SIGMA_FLOW, sigma_gyro=SIGMA_GYRO, q=0.0, p0=scaled_p0(pattern, scale), b0=B0)
            state = np.stack([br.initial_state(s)] * 3)
            for k, (x, u, d, nrm, om0, v, om) in enumerate(scenes):
                raw = np.where(s["p0"] > 0, om + BIAS, om + s["b0"])
                out, new = gpu_ctx.gyro_bias_step(variant, x, u, d=d, nrm=nrm, omega=raw, state=state, gyro_bias=setting_of(ofk, s))
                for b in range(3):
                    tag = f"n {n} variant {variant} p0 {scale:g} {pattern} step {k} problem {b}"
                    ref, j = br.step(s, state[b], variant, x[b], u[b], d[b], nrm[b], raw[b], v_s=out[b, :3], rss_s=out[b, 3], rank=out[b, 4])
                    assert ref[18] == 0 and ref[20] == k + 1, (tag, ref[18:22])
                    before = SEEN["dev"]; SEEN["dev"] = 0.0
                    try:
                        assert_bias_close(new[b], ref, tag)
                    finally:
                        worst = max(worst, SEEN["dev"]); SEEN["dev"] = max(before, SEEN["dev"])
                    P = jr.untri(new[b, 3:9])
                    assert_psd(P, tag)
                    if pattern == "mixed":
                        assert new[b, 0] == B0[0] and same(new[b, 3:6], np.zeros(3)), (tag, new[b, 0:9])
                state = new
    print(f"n {n} variant {variant}: largest deviation of (b^, P) over the prior scales {worst:.3e} (TOL_BIAS {TOL_BIAS:.2e})")


def test_a_prior_whose_square_is_not_finite_is_refused(gpu_ctx, ofk):
    x, u, d, nrm, om0, v, om = jr.scene(8, 5)
    wide = ofk.gyro_bias_setting(True, jr.SIGMA_FLOW, SIGMA_GYRO, 0.0, (1e-2, 1e160, 1e-2), B0)
    state = br.initial_state(br.setting(p0=1e-2, b0=B0))
    with pytest.raises(ofk.OfkError) as e:
        gpu_ctx.gyro_bias_step(ofk.SOLVE_NODE, x, u, d=d, nrm=nrm, omega=om0, state=state, gyro_bias=wide)
    assert e.value.code == ofk.E_INVALID and "p0[1]" in str(e.value), str(e.value)
    before = gpu_ctx.get_gyro_bias()
    with pytest.raises(ofk.OfkError) as e:
        gpu_ctx.set_gyro_bias(wide)
    assert e.value.code == ofk.E_INVALID and "p0[1]" in str(e.value), str(e.value)
    assert bytes(gpu_ctx.get_gyro_bias()) == bytes(before)       # the previous setting stays in place


# ---------------------------------------------------------------------------------------------------- the stage entry: flags
FLAG_CASES = ("negative P", "NaN omega", "inf omega", "NaN bias", "one point", "two points", "two equal points", "no valid point", "collinear")
STAYS = ("negative P", "NaN bias")                               # the degenerate thing is the state itself: a good step meets it again


def mixed_batch(name):
    """Three problems of 65 points of which only problem 1 is `name`'s; problems 0 and 2 and the all-good batch are jr.scene's.
    Returns the good batch, the batch, both as dicts of gyro_bias_step's arrays, and the states."""
    s = br.setting(**DEGENERATE_SETTING)
    sc = [jr.scene(65, 11 + 7 * b) for b in range(3)]
    x, u, d, nrm = (np.stack([c[i] for c in sc]) for i in range(4))
    raw = np.stack([c[6] for c in sc]) + BIAS
    good = dict(x=x, u=u, d=d, nrm=nrm, omega=raw, valid=np.ones((3, 65), np.uint8))
    prob, override, flag, kept = degenerate_cases()[name]
    bad = {k: v.copy() for k, v in good.items()}
    bad["omega"][1] = prob["raw"]
    m = len(prob["x"])
    if prob["valid"] is not None:
        bad["valid"][1] = prob["valid"]
    elif m < 65:                                                 # the case's points in front, the rest of the row masked
        bad["x"][1, :m] = prob["x"]; bad["u"][1, :m] = prob["u"]; bad["valid"][1, m:] = 0
    state = np.stack([br.initial_state(s)] * 3)
    state[1] = degenerate_state(s, override)
    return s, good, bad, state, flag, kept


def step_of(ctx, ofk, s, a, state, variant=jr.NODE):
    return ctx.gyro_bias_step(variant, a["x"], a["u"], d=a["d"], nrm=a["nrm"], omega=a["omega"], state=state, valid=a["valid"], gyro_bias=setting_of(ofk, s))


def reference_of(s, a, state, out, b, variant=jr.NODE):
    return br.step(s, state[b], variant, a["x"][b], a["u"][b], a["d"][b], a["nrm"][b], a["omega"][b], valid=a["valid"][b], v_s=out[b, :3], rss_s=out[b, 3],
                   rank=out[b, 4])[0]


def assert_flagged(rec, ref, state, q, tag):
    """A flagged record against the reference's: b^ and the predicted P to the bit, the zeros, the counters, the omegas."""
    assert rec[18] == ref[18] != 0, (tag, rec[18], ref[18])
    assert same(rec[0:3], state[0:3]) and same(rec[0:3], ref[0:3]), (tag, "b^", rec[0:3], state[0:3])
    predicted = state[3:9].copy()
    predicted[q > 0] += q[q > 0]                                 # the estimated axes' diagonal; nothing else is written
    assert same(rec[3:9], predicted) and same(rec[3:9], ref[3:9]), (tag, "P is the prediction", rec[3:9], predicted)
    assert not rec[15:18].any() and rec[19] == 0 and not rec[22:28].any() and not rec[29:].any(), (tag, rec)
    assert np.array_equal(rec[[20, 21, 28]], ref[[20, 21, 28]]) and rec[20] == state[20] and rec[21] == state[21] + 1, (tag, rec[[20, 21, 28]], ref[[20, 21, 28]])
    assert same(rec[9:12], ref[9:12]) and np.array_equal(rec[12:15], ref[12:15], equal_nan=True), (tag, rec[9:15], ref[9:15])


@pytest.mark.parametrize("name", FLAG_CASES)
def test_stage_entry_degenerate_problem_in_a_batch(gpu_ctx, ofk, name):
    s, good, bad, state, flag, kept = mixed_batch(name)
    q = np.where(np.array([1, 0, 0, 0, 0, 1], bool), s["q"], 0.0)
    gstate = np.stack([br.initial_state(s)] * 3)
    gout, gnew = step_of(gpu_ctx, ofk, s, good, gstate)
    assert np.all(gnew[:, 18] == 0)
    out, new = step_of(gpu_ctx, ofk, s, bad, state)
    ref = reference_of(s, bad, state, out, 1)
    assert ref[18] == flag and ref[28] == kept, (name, "the reference's flag", ref[18], flag, ref[28])
    assert_flagged(new[1], ref, state[1], q, name)
    if name in ("NaN omega", "inf omega", "NaN bias"):
        assert not np.all(np.isfinite(new[1, 12:15])), (name, new[1, 12:15])
    for b in (0, 2):                                             # the neighbours never hear of it
        assert same(new[b], gnew[b]) and same(out[b], gout[b]), (name, b)
    # a good step from the flagged state
    sc = [jr.scene(65, 300 + b) for b in range(3)]
    nxt = dict(x=np.stack([c[0] for c in sc]), u=np.stack([c[1] for c in sc]), d=good["d"], nrm=good["nrm"], omega=np.stack([c[6] for c in sc]) + BIAS,
               valid=np.ones((3, 65), np.uint8))
    out2, new2 = step_of(gpu_ctx, ofk, s, nxt, new)
    for b in range(3):
        r2 = reference_of(s, nxt, new, out2, b)
        tag = f"{name}: the step behind, problem {b}"
        if b == 1 and name in STAYS:
            assert r2[18] == flag, (tag, r2[18])
            assert_flagged(new2[1], r2, new[1], q, tag)
        else:
            assert r2[18] == 0 and r2[20] == new[b, 20] + 1 and r2[21] == 2, (tag, r2[18:22])
            assert_bias_close(new2[b], r2, tag)
    print(f"{name}: flag {int(new[1, 18])}, kept {int(new[1, 28])}; behind it flag {int(new2[1, 18])}")


@pytest.mark.parametrize("n", (1, 2))
def test_stage_entry_below_three_points(gpu_ctx, ofk, n):
    s = br.setting(**DEGENERATE_SETTING)
    sc = [jr.scene(65, 11 + 7 * b) for b in range(3)]
    a = dict(x=np.stack([c[0][:n] for c in sc]), u=np.stack([c[1][:n] for c in sc]), d=np.stack([c[2] for c in sc]), nrm=np.stack([c[3] for c in sc]),
             omega=np.stack([c[6] for c in sc]) + BIAS, valid=np.ones((3, n), np.uint8))
    state = np.stack([br.initial_state(s)] * 3)
    out, new = step_of(gpu_ctx, ofk, s, a, state)
    for b in range(3):
        ref = reference_of(s, a, state, out, b)
        assert ref[18] == n and ref[28] == n, (n, b, ref[18], ref[28])         # one point: the solve does not solve; two: it does, the core cannot
        assert_flagged(new[b], ref, state[b], np.array([s["q"], 0, 0, 0, 0, s["q"]]), f"n {n} problem {b}")


# ---------------------------------------------------------------------------------------------------- the stage entry: wide batches
def three_problems():
    sc = [jr.scene(8, 40 + b) for b in range(3)]
    s = br.setting(sigma_flow=jr.SIGMA_FLOW, sigma_gyro=SIGMA_GYRO, q=1e-10, p0=(1e-2, 5e-3, 2e-2), b0=B0)
    state = np.stack([br.initial_state(s)] * 3)
    state[1, 0:3] = [-2e-3, 1e-3, 3e-3]; state[1, 3:9] = [2e-4, 1e-5, 0, 3e-4, -2e-5, 1e-4]; state[1, 20:22] = 5
    state[2, 0:3] = [4e-3, 0.0, -1e-3]; state[2, 3:9] = [1e-6, 0, 0, 4e-6, 0, 9e-6]; state[2, 20:22] = (2, 3)
    raw = np.stack([c[6] for c in sc]) + BIAS * np.array([[1.0], [-1.0], [0.5]])
    return s, dict(x=np.stack([c[0] for c in sc]), u=np.stack([c[1] for c in sc]), d=np.stack([c[2] for c in sc]) * [1.0, 1.2, 0.8],
                   nrm=np.stack([c[3] for c in sc]), omega=raw, valid=np.ones((3, 8), np.uint8)), state


def tiled(a, state, B):
    idx = np.arange(B) % 3
    return {k: np.ascontiguousarray(v[idx]) for k, v in a.items()}, np.ascontiguousarray(state[idx])


@pytest.mark.parametrize("B", (64, 65, 130, 257))
def test_stage_entry_wide_batches(gpu_ctx, ofk, B):
    """k_gyro_bias_apply is one thread per problem in blocks of 64: a full block, one past it, two blocks and a bit, five."""
    s, a, state = three_problems()
    out3, new3 = step_of(gpu_ctx, ofk, s, a, state)
    assert np.all(new3[:, 18] == 0) and not same(new3[0], new3[1]) and not same(new3[1], new3[2]) and not same(out3[0], out3[2])
    for b in range(3):
        assert_bias_close(new3[b], reference_of(s, a, state, out3, b), f"batch 3 problem {b}")
    wa, wstate = tiled(a, state, B)
    out, new = step_of(gpu_ctx, ofk, s, wa, wstate)
    for b in range(B):
        assert same(new[b], new3[b % 3]) and same(out[b], out3[b % 3]), (B, b, new[b], new3[b % 3])


def test_stage_entry_wide_batch_with_the_robust_setting(gpu_ctx, ofk):
    """The robust solve draws its hypotheses per problem index, so problem b is not problem b % 3 here: every problem is held to the
    robust solve at the host's omega - b^ (bits) and to the reference under that solve's weights."""
    B, n = 65, 65
    sc = [jr.scene(n, 50 + b, outliers=True) for b in range(3)]
    idx = np.arange(B) % 3
    x, u, d, nrm = (np.stack([sc[i][k] for i in idx]) for k in range(4))
    raw = np.stack([sc[i][4] for i in idx])
    rob = ofk.robust_setting("tukey", hypotheses=32, seed=77)
    s = br.setting(sigma_flow=jr.SIGMA_FLOW, sigma_gyro=SIGMA_GYRO, q=1e-10, p0=1e-2, b0=B0)
    state = np.stack([br.initial_state(s)] * B)
    state[:, 0:3] = state[:, 0:3] * (1.0 + 0.25 * idx[:, None])
    out, new = gpu_ctx.gyro_bias_step(ofk.SOLVE_NODE, x, u, d=d, nrm=nrm, omega=raw, state=state, robust=rob, gyro_bias=setting_of(ofk, s))
    out_r, w, st = gpu_ctx.velocity_solve_robust(ofk.SOLVE_NODE, x, u, d=d, nrm=nrm, omega=raw - state[:, 0:3], robust=rob)
    assert same(out, out_r) and np.any((w > 0) & (w < 1))
    for b in range(B):
        ref, j = br.step(s, state[b], jr.NODE, x[b], u[b], d[b], nrm[b], raw[b], w=w[b], v_s=out[b, :3], rss_s=out[b, 3], rank=out[b, 4])
        assert ref[18] == 0 and new[b, 28] == np.count_nonzero(w[b] > 0), (b, ref[18])
        assert_bias_close(new[b], ref, f"robust batch {B} problem {b}")


# ---------------------------------------------------------------------------------------------------- streams: steps that do not solve
KEYS = ("rec", "fused", "x", "P", "tracks", "counts", "nxt", "keep", "bias")


def assert_stream_same(a, b, s, tag, sb=None):
    """Stream s of run a carries the bits of stream sb (default s) of run b, step by step: every output and the bias record."""
    sb = s if sb is None else sb
    for t, (x, y) in enumerate(zip(a, b)):
        for k in KEYS:
            if x[k] is not None:
                assert np.array_equal(bits(np.ascontiguousarray(x[k][s])), bits(np.ascontiguousarray(y[k][sb]))), (tag, t, k, x[k][s], y[k][sb])


def predicted_state(before, kw):
    """(b^, P) of a step that only predicts: q on the estimated axes' diagonal."""
    st = np.array(before[0:9], np.float64)
    est = np.broadcast_to(np.asarray(kw["p0"], np.float64), (3,)) > 0
    st[[3, 6, 8]] += np.where(est, kw["q"], 0.0)
    return st


GAPS = [pytest.param(f, None, "range", id=f"range-{f}") for f in ssr.FUSIONS]
GAPS += [pytest.param("replace", "tukey", "range", id="range-replace-robust"), pytest.param("plain", None, "gyro", id="gyro-plain"),
         pytest.param("replace", None, "gyro", id="gyro-replace")]


@pytest.mark.parametrize("fusion_name,robust,what", GAPS)
def test_stream_step_that_does_not_solve(ofk, fusion_name, robust, what):
    """Stream 1's range (or, where the sensors' omega is read, its second gyro axis) is NaN at the first step only."""
    kw = bias_keywords()
    how = dict(drop=1) if what == "range" else dict(nan_gyro=1)
    a, b = twin(ofk, fusion_name, kw, robust=robust, **how)      # the twin holds across the gap; every step passes the reference
    clean, _ = run(ofk, fusion_name, bias=kw, robust=robust)
    start = br.initial_state(br.setting(**kw))
    gap = a[0]["bias"][1]
    assert clean[0]["bias"][1, 18] == 0 and clean[0]["rec"][1, 4] == 3
    assert gap[18] == 1 and a[0]["rec"][1, 4] == 0, (gap[18], a[0]["rec"][1])
    assert same(gap[0:9], predicted_state(start, kw)) and gap[20] == 0 and gap[21] == 1, gap
    assert not gap[15:18].any() and gap[19] == 0 and not gap[22:28].any()
    assert_stream_same(a, clean, 0, f"{fusion_name} {what}: stream 0")
    for st, t in ((a[1], 2), (a[2], 3)):                         # behind the gap
        assert np.all(st["bias"][:, 18] == 0) and np.array_equal(st["bias"][:, 20], [t, t - 1]) and np.all(st["bias"][:, 21] == t), st["bias"][:, 18:22]
    print(f"{fusion_name} robust {robust} NaN {what}: flags {[st['bias'][:, 18].tolist() for st in a]}; largest deviation so far {SEEN['dev']:.3e}")


@pytest.mark.parametrize("fusion_name", ("plain", "replace"))
def test_stream_without_tracks(ofk, fusion_name):
    """Stream 1 starts from a uniform frame: no corner, no track, nothing to solve."""
    kw = bias_keywords()
    # replace re-detects in front of the tracker, so its second step solves on corners this run never saw: no reference there
    a, b = twin(ofk, fusion_name, kw, blank=1, reference=fusion_name == "plain")
    clean, _ = run(ofk, fusion_name, bias=kw)
    assert a[0]["n"][1] == 0 and a[0]["n"][0] > 10, a[0]["n"]
    state = br.initial_state(br.setting(**kw))
    empty = 0
    for t, st in enumerate(a):
        rec = st["bias"][1]
        if st["n"][1] == 0 and (fusion_name == "plain" or t == 0):
            empty += 1
            assert rec[18] == 1 and rec[28] == 0 and same(rec[0:9], predicted_state(state, kw)) and rec[20] == state[20] and rec[21] == t + 1, (t, rec)
        state = rec
    assert empty == (2 if fusion_name == "plain" else 1), empty
    if fusion_name == "replace":                                 # the fresh corners of the previous frame: solved, updated
        rec = a[1]["bias"][1]
        assert a[1]["rec"][1, 15] == 1 and rec[18] == 0 and rec[28] > 10 and rec[20] == 1 and rec[21] == 2, rec[18:29]
    assert a[-1]["bias"][1, 18] == 0 and a[-1]["bias"][1, 21] == 3
    assert_stream_same(a, clean, 0, f"{fusion_name}: stream 0 beside a stream without tracks")
    print(f"{fusion_name}: {empty} steps without tracks, flags of stream 1 {[st['bias'][1, 18] for st in a]}")


def test_hold_on_skip_holds_the_bias_too(ofk):
    import dataclasses
    fusion = dataclasses.replace(ssr.make_fusion("ekf6"), hold_on_skip=True)
    assert fusion.use_imu and fusion.filter and fusion.flow == ofk.FLOW_LK
    kw = bias_keywords()
    a, b = twin(ofk, "ekf6", kw, B=1, drop=2, fusion=fusion)     # assert_twin: the IMU state's omega is the raw one behind every step
    held = a[1]
    assert held["rec"][0, 15] == 0 and held["fused"][0, 7] == 0 and held["bias"][0, 18] == 1, (held["rec"][0], held["bias"][0, 18:22])
    assert same(held["bias"][0, 0:9], predicted_state(a[0]["bias"][0], kw)) and held["bias"][0, 20] == 1 and held["bias"][0, 21] == 2
    assert same(held["imu_after"][:, 18:21], held["raw"])
    assert np.array_equal(bits(held["tracks"]), bits(a[0]["tracks"])) and np.array_equal(held["counts"], a[0]["counts"])      # held: the old tracks
    after = a[2]["bias"][0]
    assert after[18] == 0 and after[20] == 2 and after[21] == 3 and not same(after[0:3], held["bias"][0, 0:3]), after[18:22]


@pytest.mark.parametrize("robust", (None, "tukey"))
def test_fused_step_below_min_solve_does_not_update(ofk, robust):
    """A fused step whose kept points do not exceed ofk_fusion.min_solve is not solved (record[15] == 0) whatever rank its matrix has:
    a stream step that is not solved is "not attempted" (include/ofk.h), here for the whole run, plain and robust fused kernel."""
    import dataclasses
    fusion = dataclasses.replace(ssr.make_fusion("replace"), min_solve=1000)
    kw = bias_keywords()
    a, b = twin(ofk, "replace", kw, fusion=fusion, robust=robust)
    state = np.stack([br.initial_state(br.setting(**kw))] * 2)
    for t, st in enumerate(a):
        assert not st["rec"][:, 15].any() and not st["fused"][:, 7].any() and np.all(st["n"] > 10), (t, st["rec"][:, 15], st["n"])
        for s in range(2):
            rec = st["bias"][s]
            assert rec[18] == 1 and same(rec[0:9], predicted_state(state[s], kw)) and rec[20] == 0 and rec[21] == t + 1, (t, s, rec)
        state = st["bias"]
    print(f"min_solve above the count: rank of the unsolved records {[st['rec'][:, 4].tolist() for st in a]}")


# ---------------------------------------------------------------------------------------------------- streams: wide batches
RESET2 = np.array([[2e-4, -1e-4, 1e-4, 2.5e-5, 0, 0, 2.5e-5, 0, 2.5e-5], [-1e-3, 5e-4, 2e-3, 4e-5, 1e-6, 0, 1e-5, -2e-6, 9e-5]])
_two = {}


def two_streams(ofk, fusion_name):
    if fusion_name not in _two:
        _two[fusion_name] = run(ofk, fusion_name, bias=bias_keywords(), reset=RESET2, steps_n=2)[0]
    return _two[fusion_name]


@pytest.mark.parametrize("fusion_name", ("plain", "ekf6"))
@pytest.mark.parametrize("B", (65, 130))
def test_stream_wide_batches(ofk, B, fusion_name):
    """k_gyro_bias_apply (and under use_imu its restore) past one 64-thread block; k_stream_bias one workgroup per stream."""
    base = two_streams(ofk, fusion_name)
    assert np.all(base[-1]["bias"][:, 18] == 0) and not same(base[-1]["bias"][0], base[-1]["bias"][1])
    wide, fusion = run(ofk, fusion_name, bias=bias_keywords(), reset=RESET2[np.arange(B) % 2], steps_n=2, B=B)
    for s in range(B):
        assert_stream_same(wide, base, s, f"{fusion_name} batch {B} stream {s}", s % 2)
    if fusion is not None and fusion.use_imu:
        for t, st in enumerate(wide):
            assert same(st["imu_after"][:, 18:21], st["raw"]), (B, t, "the IMU state's omega is the raw one again")
            assert same(st["imu_after"], base[t]["imu_after"][np.arange(B) % 2]), (B, t)


# ---------------------------------------------------------------------------------------------------- streams: beside the other settings
def other_settings():
    from of_amd.pipeline import CameraModel
    import combined_cases as cc
    s = {"cov": (dict(cov="propagate", sigma_flow_px=0.3, sigma_pos_px=0.5, sigma_d=0.04, cov_filter=True, r_floor=1e-8), True),
         "plane": (dict(plane=True), False),
         "zones": (dict(cc.ZONES), True),
         "gate": (dict(cc.GATE), True),
         "grid": (dict(grid_cell=20, grid_cap=1, grid_max_rank=0), True),            # 8 x 6 cells of one corner for 64 corners asked
         "camera": (dict(camera=CameraModel(model="brown", fx=200.0, fy=200.0, cx=80.0, cy=60.0, k=(-0.05, 0.01, 0.0, 0.0))), False)}
    every = {}
    for name, (extra, _) in s.items():
        if name != "plane":                                      # the plane solve is refused beside the covariance: both take the normal as an input
            every.update(extra)
    s["all"] = (every, False)
    return s


@pytest.mark.parametrize("name", ("cov", "plane", "zones", "gate", "grid", "camera", "all"))
def test_twin_run_beside_the_other_settings(ofk, name):
    """ekf6: the resident IMU state, the filter (behind the covariance's deferred correct) and the restore launch."""
    extra, reference = other_settings()[name]
    a, b = twin(ofk, "ekf6", bias_keywords(b0=(2e-3, -1e-3, 1e-3)), extra=extra, reference=reference)
    print(f"{name}: flags {[st['bias'][:, 18].tolist() for st in a]}, tracked {[st['n'].tolist() for st in a]}")
    assert all(np.all(np.isin(st["bias"][:, 18], (0, 1, 2))) for st in a) and a[-1]["bias"][0, 21] == 3


# ---------------------------------------------------------------------------------------------------- facades
def test_facades_return_the_context_step(pkg, ofk):
    import of_amd.simulation as sim
    import of_amd.velocity_node as node
    x, u, d, nrm, om0, v, om = jr.scene(65, 3)
    kw = dict(sigma_flow=jr.SIGMA_FLOW, sigma_gyro=SIGMA_GYRO, q=1e-10, p0=(1e-2, 0.0, 5e-3), b0=tuple(B0))
    ctx = ofk.default_context()
    state = None
    for k in range(2):
        vn, R, rank, s_, st = node.gyro_bias_step(x, u, d, nrm, om0, state=state, **kw)
        out, want = ctx.gyro_bias_step(ofk.SOLVE_NODE, x, u, d=d, nrm=nrm, omega=om0, state=state, **kw)
        assert same(st, want) and same(vn, out[:3]) and rank == 3 and same(R, out[3:4]) and st[18] == 0 and st[21] == k + 1
        vs, R, s_, st2 = sim.gyro_bias_step(x, u, d, nrm, om0, state=state, **kw)
        out, want = ctx.gyro_bias_step(ofk.SOLVE_SIM, x, u, d=d, nrm=nrm, omega=om0, state=state, **kw)
        assert same(st2, want) and same(vs, out[:3]) and same(R, out[3:4]) and st2[18] == 0
        state = st


def test_optical_fusion_fills_last_gyro_bias(pkg, ofk):
    from of_amd import synth
    from of_amd import velocity_node as node
    frames, info = synth.render_sequence(480, 640, 31, 3, v=(0.01, -0.008, 0.004), omega=(0, 0, 0), d=0.75, scaling=0.01)
    m = node.optical_fusion(spin=False, synthetic_test=False, gyro_bias=dict(sigma_flow=0.2, sigma_gyro=2e-5, q=1e-12, p0=1e-2, b0=(1e-4, 0.0, -1e-4)))
    m.feature_params = dict(qualityLevel=0.05, minDistance=10, blockSize=12)
    m.T = 2.0
    assert m.last_gyro_bias is None
    seen = []
    for t in range(3):
        m.call_optical(frames[t])
        if t:
            assert m.step() is not None
            rec = m._stream.gyro_bias()[0]
            assert m.last_gyro_bias is not None and same(m.last_gyro_bias, rec) and rec[21] == t, (t, rec)
            seen.append(rec.copy())
    assert same(seen[0][12:15], seen[0][9:12] - np.array([1e-4, 0.0, -1e-4])) and same(seen[1][12:15], seen[1][9:12] - seen[0][0:3])
    plain = node.optical_fusion(spin=False, synthetic_test=False)
    assert plain.last_gyro_bias is None
