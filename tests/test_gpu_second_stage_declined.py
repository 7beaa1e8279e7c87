"""GPU: the second-stage solves (joint, plane, epipolar, covariance) in the resident forms where they do NOT take over - the path a
hover takes on every step.  include/ofk.h promises the same for all four when the second stage declines (flag 1, 2 or 3) or the step
itself did not solve (record[15] == 0): the record is untouched bit for bit, the second-stage record reports the flag with the slots
the header names set to zero, the filter is corrected with the plain solve's v where the step solved and stays at its prediction
where it did not, fused[7] says which, and vel_overwrite is not repeated.  The other suites enter the resident forms on success only.

Every case compares a run with the setting on against a run with the same inputs and the setting off - records, fused rows, filter
state, IMU state, tracks, counts, next points and keep flags are the same bits - and the second-stage record against the reference
(tests/joint_reference.py, plane_reference.py, epi_reference.py, cov_reference.py) fed with the downloaded points: the flag is
asserted on the reference first, so no case asks the device which way a gate falls.  For the sigma_max levers the reference's
predicted sigma exceeds the gate by a factor of 2 at least (asserted).  Slots that stay set in a flagged record are held to the
existing REC_TOL / RSS_TOL (tests/joint_checks.py, tests/plane_checks.py); no tolerance is introduced here.

  a  an unsolved step: stream 1's range is NaN at the first step only, so that the setting-off run is in the same state there
     (joint, plane, epipolar, covariance x the four fusions, and the robust solve with a filter, which takes the deferred leg of
     k_stream_fuse_robust).  Stream 0 has the bits of the run without the dropout; the step behind the gap passes the ordinary check
     against the reference and the filter's reference chain carries the prediction through the gap.
  b  solved but declined, the whole batch, by a lever of the setting: sigma_max far below the predicted sigma (flag 2), an anchor of
     1e-6 px or an anchor_min above the corner count (flag 3), a beam at right angles to the optical axis (flag 1), a prior term that
     overflows (flag 1) - on stream steps and on pairs (batch 2 and 130, one and two slices, the second-stage records the same bits
     across the forms, ofk_pairs_filter_step behind the run giving the setting-off state).
  c  a mixed batch: only problem 1 declines - by its sensors' normal (1, 0, 0), which makes n0.e zero, and (stream steps) by a hover
     clip, rendered with v = 0, that the default gates must stop with the same factor of 2.  Problem 0 passes the ordinary flag-0
     check and has the bits of a run where both problems are good.  The joint solve has no per-problem lever short of a two-point
     image: its mixed batch is (a)'s dropout, which already mixes flag 1 with flag 0.

The clips and pairs are tests/test_gpu_joint.py's (120 x 160, 64 corners, 2 streams, 2 steps); (c) renders them with
v = (0.012, -0.009, 0.004), tests/test_gpu_plane.py's, at which the plane solve of problem 0 passes its default gate.
Printed per case for the summary: the flag reached and, for flag 2, the reference's sigma-to-gate ratio."""
import numpy as np
import pytest

import cov_reference as cr
import second_stage_runs as ss
from joint_checks import JOINT, SEEN as JOINT_SEEN, assert_joint_close
from oracle import estimation_oracle as eo
from plane_checks import PLANE, SEEN as PLANE_SEEN, assert_plane_close
from point_stage_helpers import bits
from second_stage_runs import CORNERS, FUSIONS
from test_gpu_cov import SIG_PX, SEEN as COV_SEEN, assert_cov_close
from test_gpu_epi import EPI, SEEN as EPI_SEEN, assert_epi_close

pytestmark = pytest.mark.gpu

COV = dict(SIG_PX, mode="propagate", filter_r=True, r_floor=1e-8)
SETTINGS_A = dict(joint=JOINT, plane=dict(PLANE, sigma_max=np.inf), epi=EPI, cov=COV)      # open gates: the step behind the gap succeeds
DROP, T_A = 1, 3                                                 # two steps, the range drops out at the first: nothing the setting rewrote lies before it
_off = {}


def run_off(ofk, fusion_name, **kw):
    """The setting-off run of a configuration, rendered and run once."""
    key = (fusion_name,) + tuple(sorted((k, repr(v)) for k, v in kw.items()))
    if key not in _off:
        _off[key] = ss.stream_run(ofk, None, fusion_name, **kw)
    return _off[key]


def check_solved(ofk, second, st, s, fusion, before, tag, want=0):
    """The ordinary check of a step's second-stage record against the reference, which must reach flag `want`."""
    kind = second[0]
    n = int(st["n"][s])
    rec, (rec2, rows) = st["rec"][s], ss.second_of(st, s)
    ref = ss.step_reference(ofk, second, st, s, st["sr"][s], fusion, before)
    assert ref["flag"] == want and before[4] == 3, (tag, ref["flag"], ref["rec"][10:18])
    if kind == "joint":
        assert_joint_close(rec[0:3], rec[3], rec2, ref, tag)
    elif kind == "plane":
        assert_plane_close(rec[0:3], rec[3], rec2, ref, tag)
    else:
        assert_epi_close(rec[0:3], rec[3], rec2, rows[:n], ref, tag)
        assert np.all(rows[n:, 3] == 1) and not rows[n:, :3].any(), tag
    assert not np.array_equal(rec[0:3], before[0:3]), (tag, "the record was rewritten")
    return ref


def check_declined(ofk, second, st, s, fusion, before, tag, want, gated=False):
    """A step's second-stage record that carries flag `want` (asserted on the reference first); gated: flag 2 comes from sigma_max,
    which the reference's predicted sigma must exceed by a factor of 2.  Returns the reference."""
    rec, (rec2, rows) = st["rec"][s], ss.second_of(st, s)
    ref = ss.step_reference(ofk, second, st, s, st["sr"][s], fusion, before)
    assert ref["flag"] == want, (tag, "the reference's flag", ref["flag"], want, ref["rec"][10:18])
    if gated:
        ratio = ss.predicted_ratio(ofk, second, ref)
        assert ratio >= 2.0, (tag, "the predicted sigma is not twice the gate", ratio)
    ss.assert_declined(second[0], rec2, rows, ref, rec[0:3], rec[3], tag)
    return ref


def cov_record(st, s, fusion, cfgd):
    """cov_reference's record of stream s of a step."""
    n = int(st["n"][s])
    kw = {}
    if fusion is not None and fusion.use_imu:
        imu = st["imu"][s]
        kw = dict(nrm=imu[15:18], omega=imu[18:21], R=imu[6:15])
    return cr.pair_record(cr.NODE, st["old"][s, :n], st["nxt"][s, :n], None, st["sr"][s], cfgd, st["rec"][s], keep=st["keep"][s, :n].astype(bool), **kw)


def filter_chain(fusion, steps, s, cov=None):
    """The filter's reference chain over the steps of stream s: predict at every step, correct where record[15] is set.  cov: the
    covariance setting's dict (then the correct is cov_reference's, with R_eff, and the cov records are compared)."""
    m = fusion.model
    use_imu = fusion.use_imu
    loop = cr.CovStreamLoop(m, cov, fusion.z_sign, fusion.z_source) if cov is not None else None
    xk, Pk = np.array(m.x0, np.float64), np.array(m.P0, np.float64)
    for k, st in enumerate(steps):
        n = int(st["n"][s])
        tag = f"filter chain stream {s} step {k}"
        rec, sr = st["rec"][s], st["sr"][s]
        control = st["dv"][s] if use_imu else sr[25:28]
        if loop is not None:
            cv, xk, Pk, fused = loop.step(st["old"][s, :n], st["nxt"][s, :n], st["keep"][s, :n], sr, rec, control, imu=st["imu"][s] if use_imu else None)
            got = st["second"][s]
            if rec[15] != 0:
                assert cv[13] == 0, tag
                assert_cov_close(got, cv, tag)
                assert got[15] == cv[15] and abs(got[14] - cv[14]) <= 1e-9 * cv[14] and cv[14] > 0, (tag, got[14:16], cv[14:16])
            else:
                assert np.array_equal(got, cr.void_record()) and np.array_equal(cv, cr.void_record()), (tag, got)
        else:
            xk, Pk = eo.kf_predict(xk, Pk, m.F, m.Q, m.B if m.nc else None, control if m.nc else None)
            if rec[15] != 0:
                z = fusion.z_sign * (rec[8:11] if fusion.z_source else rec[0:3])
                if m.nm > 3:
                    z = np.concatenate([z, sr[22:22 + m.nm - 3]])
                xk, Pk = eo.kf_correct(xk, Pk, m.H, m.R, z)
            fused = np.zeros(8); fused[:m.ns] = xk; fused[6] = np.trace(Pk); fused[7] = 1.0 if rec[15] != 0 else 0.0
        np.testing.assert_allclose(st["x"][s], xk, rtol=1e-9, atol=1e-15, err_msg=tag)
        np.testing.assert_allclose(st["P"][s], Pk, rtol=1e-9, atol=1e-18, err_msg=tag)
        np.testing.assert_allclose(st["fused"][s], fused, rtol=1e-9, atol=1e-15, err_msg=tag)


def report(tag, flags, ratios=()):
    seen = f"joint {JOINT_SEEN['dev']:.3e} plane {PLANE_SEEN['dev']:.3e} epi {EPI_SEEN['dev']:.3e} cov {COV_SEEN['dev']:.3e}"
    r = f", sigma / gate {min(ratios):.3g} .. {max(ratios):.3g}" if len(ratios) else ""
    print(f"{tag}: flags {sorted(set(flags))}{r}; largest deviations of the flag-0 neighbours so far: {seen}")


# ---------------------------------------------------------------------------------------------------- a. an unsolved step
CASES_A = [pytest.param(k, f, None, id=f"{k}-{f}") for k in ("joint", "plane", "epi", "cov") for f in FUSIONS]
CASES_A.append(pytest.param("joint", "replace", "tukey", id="joint-replace-robust"))


@pytest.mark.parametrize("kind,fusion_name,robust", CASES_A)
def test_unsolved_step(pkg, ofk, kind, fusion_name, robust):
    second = (kind, SETTINGS_A[kind])
    kw = dict(T=T_A, robust=robust) if robust else dict(T=T_A)
    off, _, _ = run_off(ofk, fusion_name, drop=DROP, **kw)
    steps, sensors, fusion = ss.stream_run(ofk, second, fusion_name, drop=DROP, **kw)
    clean, _, _ = ss.stream_run(ofk, second, fusion_name, **kw)
    assert len(steps) == 2
    for k, (a, b) in enumerate(zip(steps, clean)):               # stream 0 never hears of the dropout
        ss.assert_same_state(a, b, 0, f"stream 0 step {k}")
        for x, y in zip(ss.second_of(a, 0), ss.second_of(b, 0)):
            assert (x is None and y is None) or np.array_equal(bits(x), bits(y)), (k, x, y)
    k = DROP - 1
    st, tag = steps[k], f"{kind} {fusion_name} the unsolved step"
    ss.assert_same_state(st, off[k], 1, tag)
    rec, (rec2, rows) = st["rec"][1], ss.second_of(st, 1)
    assert rec[15] == 0 and rec[4] == 0 and not rec[0:4].any() and clean[k]["rec"][1, 4] == 3, (tag, rec)
    if fusion is not None:
        assert st["fused"][1, 7] == 0, (tag, st["fused"][1])
    if fusion is not None and fusion.filter:                     # the filter stays at its prediction
        m = fusion.model
        px, pP = (steps[k - 1]["x"][1], steps[k - 1]["P"][1]) if k else (np.array(m.x0, np.float64), np.array(m.P0, np.float64))
        control = st["dv"][1] if fusion.use_imu else st["sr"][1, 25:28]
        xp, Pp = eo.kf_predict(px, pP, m.F, m.Q, m.B if m.nc else None, control if m.nc else None)
        np.testing.assert_allclose(st["x"][1], xp, rtol=1e-12, atol=1e-15, err_msg=tag)
        np.testing.assert_allclose(st["P"][1], Pp, rtol=1e-12, atol=1e-18, err_msg=tag)
        assert not np.allclose(clean[k]["x"][1], xp, rtol=1e-6, atol=0), (tag, "the clean run did correct")
    if kind == "cov":
        assert np.array_equal(rec2, cr.void_record()), (tag, rec2)           # void, NIS and gate 0
    else:
        ref = check_declined(ofk, second, st, 1, fusion, off[k]["rec"][1], tag, 1)
        assert np.array_equal(bits(rec2), bits(ref["rec"])), (tag, rec2, ref["rec"])       # flag 1 holds copies of inputs alone
        if kind == "epi":
            assert not rows.any(), tag
    flags = [1]
    for s in range(2):                                           # the step behind the gap: the ordinary check, both streams
        after = steps[DROP]
        assert after["rec"][s, 4] == 3 and (fusion is None or (after["rec"][s, 15] == 1 and after["fused"][s, 7] == 1)), (s, after["rec"][s])
        if kind == "cov":
            cv = cov_record(after, s, fusion, dict(COV, mode=ofk.COV_PROPAGATE))
            assert cv[13] == 0, s
            assert_cov_close(ss.second_of(after, s)[0], cv, f"cov {fusion_name} stream {s} behind the gap")
            flags.append(0)
        else:
            before = after["rec"][s].copy(); before[0:4] = ss.second_of(after, s)[0][6:10]
            flags.append(check_solved(ofk, second, after, s, fusion, before, f"{kind} {fusion_name} stream {s} behind the gap")["flag"])
        if fusion is not None and fusion.filter:
            filter_chain(fusion, steps, s, dict(COV, mode=ofk.COV_PROPAGATE) if kind == "cov" else None)
    report(f"a {kind} {fusion_name}{' robust' if robust else ''}", flags)


# ---------------------------------------------------------------------------------------------------- b. solved but declined, the whole batch
FAR = 1e-4                                                       # a gate in radians far below any predicted sigma of these clips
LEVERS = {                                                       # name -> kind, setting, the flag it must reach, the fusions it works under
    "plane-sigma_max": ("plane", dict(PLANE, sigma_max=FAR), 2, FUSIONS),
    "epi-sigma_max": ("epi", dict(EPI, sigma_max=FAR), 2, FUSIONS),
    "epi-anchor": ("epi", dict(EPI, anchor=1e-6), 3, FUSIONS),
    "epi-anchor_min": ("epi", dict(EPI, anchor_min=CORNERS + 1), 3, FUSIONS),
    "plane-beam": ("plane", dict(PLANE, beam=(1.0, 0.0, 0.0)), 1, ("plain", "replace")),     # under use_imu the IMU's normal has an x component
    "epi-beam": ("epi", dict(EPI, beam=(1.0, 0.0, 0.0)), 1, FUSIONS),
    "joint-overflow": ("joint", dict(sigma_flow=0.2, sigma_omega=1e-160), 1, FUSIONS),
    "plane-overflow": ("plane", dict(sigma_flow=0.2, sigma_normal=1e-160), 1, FUSIONS),
}
CASES_B = [pytest.param(name, f, id=f"{name}-{f}") for name, lv in LEVERS.items() for f in lv[3]]


@pytest.mark.parametrize("lever,fusion_name", CASES_B)
def test_declined_stream_steps(pkg, ofk, lever, fusion_name):
    kind, setting, want, _ = LEVERS[lever]
    second = (kind, setting)
    off, _, _ = run_off(ofk, fusion_name)
    steps, sensors, fusion = ss.stream_run(ofk, second, fusion_name)
    assert len(steps) == 2
    ratios = []
    for k, st in enumerate(steps):
        for s in range(2):
            tag = f"{lever} {fusion_name} stream {s} step {k}"
            ss.assert_same_state(st, off[k], s, tag)
            assert st["rec"][s, 4] == 3, tag
            if fusion is not None:
                assert st["rec"][s, 15] == 1 and st["fused"][s, 7] == 1, (tag, st["rec"][s, 15], st["fused"][s])
            ref = check_declined(ofk, second, st, s, fusion, off[k]["rec"][s], tag, want, gated=want == 2)
            if want == 2:
                ratios.append(ss.predicted_ratio(ofk, second, ref))
    report(f"b stream {lever} {fusion_name}", [want], ratios)


_pairs_off = {}


def pairs_off(ofk, B, slices, **kw):
    key = (B, slices) + tuple(sorted((k, repr(v)) for k, v in kw.items()))
    if key not in _pairs_off:
        _pairs_off[key] = ss.pairs_run(ofk, B, None, slices, **kw)
    return _pairs_off[key]


FORMS = ((2, 1), (130, 1), (2, 2), (130, 2))                     # a workgroup per pair, a wave per pair; one and two slices


def assert_pairs_untouched(out, x, P, off, b, tag):
    """Pair b of a run against the setting-off run: records, points, status, and the filter behind ofk_pairs_filter_step."""
    for k in ("records", "prev_pts", "next_pts", "status", "err", "counts"):
        assert np.array_equal(bits(out[k][b]), bits(off[1][k][b])), (tag, k)
    assert np.array_equal(bits(x[b]), bits(off[3][b])) and np.array_equal(bits(P[b]), bits(off[4][b])), (tag, "the filter step", x[b], off[3][b])


@pytest.mark.parametrize("lever", LEVERS)
def test_declined_pairs(pkg, ofk, lever):
    kind, setting, want, _ = LEVERS[lever]
    second = (kind, setting)
    base = None
    ratios = []
    for B, slices in FORMS:
        off = pairs_off(ofk, B, slices)
        sensors, out, sec, x, P = ss.pairs_run(ofk, B, second, slices)
        sec = sec if isinstance(sec, tuple) else (sec,)
        base = base or sec
        for b in range(B):
            tag = f"{lever} B {B} slices {slices} pair {b}"
            assert_pairs_untouched(out, x, P, off, b, tag)
            for got, first in zip(sec, base):                    # the same bits across the launch forms
                assert np.array_equal(bits(got[b]), bits(first[b % 2])), tag
        if base is sec:
            for b in range(2):
                n = int(out["counts"][b])
                ref = ss.reference(ofk, second, out["prev_pts"][b, :n], out["next_pts"][b, :n], out["status"][b, :n], sensors[b], off[1]["records"][b])
                tag = f"{lever} pair {b}"
                assert ref["flag"] == want and off[1]["records"][b, 4] == 3, (tag, ref["flag"], ref["rec"][10:18])
                if want == 2:
                    ratios.append(ss.predicted_ratio(ofk, second, ref))
                    assert ratios[-1] >= 2.0, (tag, ratios[-1])
                rows = sec[1][b] if kind == "epi" else None
                ss.assert_declined(kind, sec[0][b], rows, ref, out["records"][b, 0:3], out["records"][b, 3], tag)
    report(f"b pairs {lever}", [want], ratios)


# ---------------------------------------------------------------------------------------------------- c. a mixed batch
MOTION_C = dict(v=(0.012, -0.009, 0.004), omega=(0.003, -0.002, 0.004), d=1.0)
SIDE = (1.0, 0.0, 0.0)                                           # a normal at right angles to the beam: n0.e == 0
PLANE_C = dict(sigma_flow=0.2, sigma_normal=0.5)                 # a hover's predicted sigma is the prior's: 0.5 against the default gate 0.1
SETTINGS_C = dict(normal=dict(plane=PLANE_C, epi=EPI), hover=dict(plane=PLANE_C, epi=dict(anchor=60.0, anchor_min=5)))     # hover: the default gates
ZERO = np.zeros(3)


@pytest.mark.parametrize("fusion_name", ("plain", "replace"))    # the fusions that read the sensors' normal
@pytest.mark.parametrize("how", ("normal", "hover"))
@pytest.mark.parametrize("kind", ("plane", "epi"))
def test_mixed_batch_stream_steps(pkg, ofk, kind, how, fusion_name):
    second = (kind, SETTINGS_C[how][kind])
    want = 1 if how == "normal" else 2
    kw = dict(T=2, gyro_off=ZERO, motion=MOTION_C)               # one step: the epipolar solve of stream 0 passes its default gate at the first
    bad = dict(normals={1: SIDE}) if how == "normal" else dict(hover=True)
    off, _, _ = run_off(ofk, fusion_name, **kw, **bad)
    steps, sensors, fusion = ss.stream_run(ofk, second, fusion_name, **kw, **bad)
    good, _, _ = ss.stream_run(ofk, second, fusion_name, **kw)   # both problems good
    st, tag = steps[0], f"{kind}-mixed {how} {fusion_name}"
    ss.assert_same_state(st, good[0], 0, tag + " stream 0")
    for x, y in zip(ss.second_of(st, 0), ss.second_of(good[0], 0)):
        assert (x is None and y is None) or np.array_equal(bits(x), bits(y)), tag
    before = st["rec"][0].copy(); before[0:4] = ss.second_of(st, 0)[0][6:10]
    assert np.array_equal(bits(before[0:8]), bits(off[0]["rec"][0, 0:8])), tag      # slots 6-9 hold the plain solve's bits
    check_solved(ofk, second, st, 0, fusion, before, tag + " stream 0")
    ss.assert_same_state(st, off[0], 1, tag + " stream 1")
    if fusion is not None:
        assert np.all(st["rec"][:, 15] == 1) and np.all(st["fused"][:, 7] == 1), tag
    ref = ss.step_reference(ofk, second, st, 1, st["sr"][1], fusion, off[0]["rec"][1])
    ratios = [ss.predicted_ratio(ofk, second, ref)] if want == 2 else []
    assert ref["flag"] == want and (want != 2 or ratios[0] >= 2.0), (tag, ref["flag"], ratios, ref["rec"][10:18])
    rec2, rows = ss.second_of(st, 1)
    ss.assert_declined(kind, rec2, rows, ref, st["rec"][1, 0:3], st["rec"][1, 3], tag + " stream 1")
    if fusion is not None and fusion.filter:
        for s in range(2):
            filter_chain(fusion, steps, s)
    report(f"c stream {kind} {how} {fusion_name}", [0, want], ratios)


@pytest.mark.parametrize("kind", ("plane", "epi"))
def test_mixed_batch_pairs(pkg, ofk, kind):
    second = (kind, SETTINGS_C["normal"][kind])
    kw = dict(gyro_off=ZERO, motion=MOTION_C)
    base = None
    for B, slices in FORMS:
        off = pairs_off(ofk, B, slices, normals={1: SIDE}, **kw)
        sensors, out, sec, x, P = ss.pairs_run(ofk, B, second, slices, normals={1: SIDE}, **kw)
        _, gout, gsec, gx, gP = ss.pairs_run(ofk, B, second, slices, **kw)          # both problems good
        sec = sec if isinstance(sec, tuple) else (sec,)
        gsec = gsec if isinstance(gsec, tuple) else (gsec,)
        base = base or sec
        for b in range(B):
            tag = f"{kind}-mixed B {B} slices {slices} pair {b}"
            for got, first in zip(sec, base):
                assert np.array_equal(bits(got[b]), bits(first[b % 2])), tag
            if b % 2:
                assert_pairs_untouched(out, x, P, off, b, tag)
            else:                                                # the good pair: the bits of the run where both are good
                for k in ("records", "prev_pts", "next_pts", "status", "err", "counts"):
                    assert np.array_equal(bits(out[k][b]), bits(gout[k][b])), (tag, k)
                assert np.array_equal(bits(x[b]), bits(gx[b])) and np.array_equal(bits(P[b]), bits(gP[b])), tag
                for got, g in zip(sec, gsec):
                    assert np.array_equal(bits(got[b]), bits(g[b])), tag
        if base is sec:
            for b in range(2):
                n = int(out["counts"][b])
                tag = f"{kind}-mixed pair {b}"
                ref = ss.reference(ofk, second, out["prev_pts"][b, :n], out["next_pts"][b, :n], out["status"][b, :n], sensors[b], off[1]["records"][b])
                assert ref["flag"] == b, (tag, ref["flag"], ref["rec"][10:18])
                rows = sec[1][b] if kind == "epi" else None
                rec = out["records"][b]
                if b == 0:
                    assert off[1]["records"][b, 4] == 3, tag
                    if kind == "plane":
                        assert_plane_close(rec[0:3], rec[3], sec[0][b], ref, tag)
                    else:
                        assert_epi_close(rec[0:3], rec[3], sec[0][b], rows[:n], ref, tag)
                    assert not np.array_equal(rec[0:3], off[1]["records"][b, 0:3]), tag
                else:
                    ss.assert_declined(kind, sec[0][b], rows, ref, rec[0:3], rec[3], tag)
    report(f"c pairs {kind} normal", [0, 1])
