"""GPU: the keyframe per stream (include/ofk.h: ofk_set_keyframe) against its restatement (tests/keyframe_reference.py).

(a) ofk_keyframe_step at the kernel's edges: counts around the 64-lane and 256-row boundaries at stride 1030, status and member
    patterns that keep all, none, a random set, only the first or only the last row of every chunk, appended rows none / some / past
    max_total, three streams per launch with their own sensors, states and step records.  key_xy, member, the counts, the flags, the
    reasons and key_step agree bit for bit; T, rms, D, pos, anchor, the angle and C_T within test_gpu_epi.py's REC_TOL of their slot
    group's scale (same sums, a Jacobi against numpy's eigh); R_acc within 1e-13 per entry of the restatement started from the R_acc
    the device was given (sin and cos come from two math libraries).  The largest deviations met are printed (-s) for the README.
(b) every refusal and fallback of the stage entry, each seen to count; an offset or an R_world that is no number.
(c) streams over rendered 128 x 160 sequences, 8 steps: ofk_stream_step with append re-detection, a JPEG step, the setting switched on
    in mid-stream; ofk_stream_step_fused with the robust drop, the replace re-detection, held steps, use_imu.  After every call the
    downloaded state and record equal the restatement fed with what the calls handed back.
(d) on against off: records, fused rows, tracks, counts, the table, the depths and the templates are the same bits.
(e) composition: beside a camera model, a rolling shutter (flow and gyro mode) or both with finite motion on (the copy path) the key
    solve read the ideal points in front of the rewrite, rebuilt on the host with ofk_undistort_points and ofk_rs_correct_points;
    beside finite motion alone the raw ones; beside a camera or a rolling shutter alone what the solve read; beside the gyro-bias
    setting it read the corrected omega.
(f) the refusals, download and reset."""
import dataclasses
import io as _io
import zlib

import numpy as np
import pytest

import keyframe_reference as K
from test_gpu_epi import REC_TOL

pytestmark = pytest.mark.gpu
DEV = dict(rec=0.0, R=0.0)                                       # the largest deviations met: record groups in units of their scale, R_acc per entry
EXACT = [3, 4, 5, 7, 8, 9, 26, 27, 28, 29, 30, 31]
GROUPS = ((0, 3), (6, 7), (10, 13), (13, 16), (16, 19), (19, 20), (20, 26))
R_TOL = 1e-13


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_record(got, want, tag):
    assert np.array_equal(bits(got[EXACT]), bits(want[EXACT])), (tag, got, want)
    for lo, hi in GROUPS:
        scale = max(np.abs(want[lo:hi]).max(), 1e-300)
        if lo in (10, 13, 16) and want[3] != 0:                  # dead-reckoned: D = pos - anchor, a difference, is held to the scale of its terms
            scale = max(np.abs(want[10:19]).max(), 1e-300)
        if np.all(np.isfinite(want[lo:hi])):
            err = float((np.abs(got[lo:hi] - want[lo:hi]) / scale).max())
            DEV["rec"] = max(DEV["rec"], err)
            assert err <= REC_TOL, (tag, lo, got[lo:hi], want[lo:hi])
        else:
            assert np.array_equal(np.isnan(got[lo:hi]), np.isnan(want[lo:hi])), (tag, lo, got[lo:hi], want[lo:hi])


def same_state(got_state, got_istate, want, tag):
    assert np.array_equal(got_istate, want["istate"]), (tag, got_istate, want["istate"])
    w = want["state"]
    if np.all(np.isfinite(w[:9])):
        err = float(np.abs(got_state[:9] - w[:9]).max())
        DEV["R"] = max(DEV["R"], err)
        assert err <= R_TOL, (tag, got_state[:9], w[:9])
    for lo, hi in ((9, 12), (12, 15)):                           # anchor, pos: each to its own scale
        scale = max(np.abs(w[lo:hi]).max(), 1e-300)
        assert (np.abs(got_state[lo:hi] - w[lo:hi]) / scale).max() <= REC_TOL, (tag, got_state[lo:hi], w[lo:hi])


def device_setting(ofk, s):
    return ofk.keyframe_setting(True, s["sigma_flow"], s["gate"], s["min_rows"], s["min_share"], s["rot_max"], s["max_age"])


@pytest.fixture(scope="module")
def ctx(ofk):
    c = ofk.Context(0, 64, 48, 3, 1100, 2)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ (a) the kernel's edges
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 513, 1030)
PATTERNS = ("all", "none", "random", "chunk-first", "chunk-last")
S_EDGE = 1030
SET = K.setting(rot_max=0.3, max_age=0)
FOC, CXY = 256.0, (80.0, 64.0)


def pattern_of(pattern, n, rng, S=S_EDGE):
    i = np.arange(S)
    st = {"all": np.ones(S, bool), "none": np.zeros(S, bool), "random": rng.uniform(size=S) < 0.6,
          "chunk-last": (i % 256 == 255) | (i == n - 1), "chunk-first": i % 256 == 0}[pattern]
    return (st * rng.integers(1, 256, S)).astype(np.uint8)       # any non-zero byte counts; rows beyond n are noise


def sensor_row(rng, d, nrm, om):
    sn = np.zeros(28)
    sn[0] = d; sn[1:4] = nrm; sn[4:7] = om; sn[7:16] = K.rotation(rng.normal(0, 0.3, 3)).ravel(); sn[16:19] = rng.normal(0, 0.05, 3)
    sn[19] = 1.0 / FOC; sn[20:22] = CXY; sn[22:25] = rng.normal(0, 0.01, 3)
    return sn


def scene(rng, S=S_EDGE, big_angle=False, noise=0.2, wild=0.05):
    """A stream some steps behind its keyframe: key points over the frame, a rotation accumulated before this step, the step's omega, a
    translation, the plane in the current axes; the next points are the key points through P_c = R P_K + T with noise and a few wild
    rows.  -> (next_pts f32 [S,2], sensors [28], state [16] with R_acc in front of the step)."""
    nrm = np.array([rng.normal(0, 0.05), rng.normal(0, 0.05), 1.0]); nrm /= np.linalg.norm(nrm)
    d = rng.uniform(0.8, 1.5)
    Rprev = K.rotation(rng.normal(0, 0.3 if big_angle else 0.02, 3))
    om = rng.normal(0, 0.01, 3)
    R = K.rotation(om) @ Rprev
    T = rng.normal(0, 0.04, 3) * d
    key = (rng.uniform(0, 1, (S, 2)) * [160, 128]).astype(np.float32)
    pk = np.concatenate([(key.astype(np.float64) - CXY) / FOC, np.ones((S, 1))], 1)
    q = pk @ R.T
    lam = (d - nrm @ T) / (q @ nrm)
    P = lam[:, None] * q + T
    nxt = P[:, :2] / P[:, 2:3] * FOC + CXY + rng.normal(0, noise, (S, 2))
    w = rng.uniform(size=S) < wild
    nxt[w] += rng.normal(0, 20.0, (int(w.sum()), 2))
    st = np.zeros(K.KEY_STATE); st[:9] = Rprev.ravel(); st[9:12] = rng.normal(0, 1, 3); st[12:15] = st[9:12] + rng.normal(0, 0.1, 3)
    return key, nxt.astype(np.float32), sensor_row(rng, d, nrm, om), st


def run_stage(ctx, ofk, cases, s, new_counts, max_total):
    """cases: per stream dict(next, status, n, sensors, vu, solved, step, state).  -> the device's (state, rec) and the restatement's."""
    st = {k: np.stack([c["state"][k] for c in cases]) for k in ("key_xy", "member", "state", "istate")}
    got, rec = ctx.keyframe_step(np.stack([c["next"] for c in cases]), np.stack([c["status"] for c in cases]), [c["n"] for c in cases],
                                 np.stack([c["sensors"] for c in cases]), np.stack([c["vu"] for c in cases]), [int(c["solved"]) for c in cases],
                                 [c["step"] for c in cases], st, new_counts=new_counts, max_total=max_total, keyframe=device_setting(ofk, s))
    want = [K.step(c["state"], c["next"], c["status"], c["n"], c["sensors"], c["vu"], c["solved"], c["step"], s,
                   None if new_counts is None else new_counts[b], max_total) for b, c in enumerate(cases)]
    return got, rec, want


def compare_stage(got, rec, want, tag):
    for b, (wst, wrec, count, _) in enumerate(want):
        assert np.array_equal(bits(got["key_xy"][b, :count]), bits(wst["key_xy"][:count])), (tag, b, "key_xy")
        assert np.array_equal(got["member"][b, :count], wst["member"][:count]), (tag, b, "member")
        same_state(got["state"][b], got["istate"][b], wst, (tag, b))
        same_record(rec[b], wrec, (tag, b))


def edge_case(rng, n, pattern, mpattern, b, variant):
    key, nxt, sn, st = scene(rng, big_angle=variant % 4 == 3)
    status, member = pattern_of(pattern, n, rng), pattern_of(mpattern, n, rng)
    live = int(np.count_nonzero(status[:n] & (member[:n] != 0) * 255))
    mk = [int(np.count_nonzero(member[:n])), 0, 2 * live + 3][variant % 3] if n else 0      # a healthy share / no keyframe / a share below min_share
    state = dict(key_xy=key, member=member, state=st, istate=np.array([3, mk, 2, 1], np.int32))
    return dict(next=nxt, status=status, n=n, sensors=sn, vu=rng.normal(0, 0.01, 3), solved=(b + variant) % 3 != 0, step=7 + b, state=state)


def check_step(ctx, ofk, ns, pattern, mpattern, appended, case, s=SET):
    rng = np.random.default_rng(zlib.crc32(repr((tuple(ns), pattern, mpattern, appended)).encode()))
    cases = [edge_case(rng, n, pattern, mpattern, b, b + len(appended) + len(pattern)) for b, n in enumerate(ns)]
    kept = [int(np.count_nonzero(c["status"][:c["n"]])) for c in cases]
    if appended == "none":
        new_counts, max_total = None, S_EDGE
    elif appended == "some":
        new_counts, max_total = [17 + b for b in range(len(ns))], S_EDGE
    else:                                                        # "clamped": more than max_total - kept, the budget cuts them
        new_counts, max_total = [40] * len(ns), min(S_EDGE, max(kept) + 5)
    got, rec, want = run_stage(ctx, ofk, cases, s, new_counts, max_total)
    compare_stage(got, rec, want, (case, tuple(ns), max_total))
    for b, (_, _, count, dg) in enumerate(want):
        extra = count - kept[b]
        if appended == "clamped":
            assert extra == max(0, min(40, max_total - kept[b])), (case, b)
        if extra > 0:
            assert not got["member"][b, kept[b]:count].any() and not got["key_xy"][b, kept[b]:count].any(), (case, b)
        if dg["rekey"] and kept[b]:
            assert got["member"][b, :kept[b]].all() and got["istate"][b, 0] == cases[b]["step"] + 1 and got["istate"][b, 1] == kept[b]
    return [w[1] for w in want]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_step_kernel_edges(ctx, ofk, pattern):
    """Every count under one status pattern and every member pattern, the three kinds of appends in turn, three streams per call."""
    groups = [COUNTS[0:3], COUNTS[3:6], COUNTS[6:9], (COUNTS[9], COUNTS[4], COUNTS[7])]
    flags, reasons = [], set()
    for m, mpattern in enumerate(PATTERNS):
        for g, ns in enumerate(groups):
            s = dict(SET, max_age=(0, 4, 40)[(g + m) % 3])
            recs = check_step(ctx, ofk, ns, pattern, mpattern, ("none", "some", "clamped")[(g + m) % 3], (pattern, mpattern, g), s)
            flags += [int(r[3]) for r in recs]
            for r in recs:
                reasons |= {q + 1 for q in range(5) if int(r[30]) >> q & 1}
    if pattern in ("all", "random"):
        assert flags.count(0) >= 6 and 2 in flags and 1 in flags, flags      # the comparison of T and C_T is not one of zeros
        assert reasons == {1, 2, 3, 4, 5}, reasons
    print("largest deviations so far: record groups", DEV["rec"], "of their scale, R_acc", DEV["R"], "per entry")


def test_three_streams_of_different_counts(ctx, ofk):
    for ns in ((1030, 0, 257), (1, 513, 64), (300, 300, 299)):
        recs = check_step(ctx, ofk, ns, "random", "all", "clamped", ("mixed", ns))
        assert sum(r[3] == 0 for r in recs) >= 1, ns
    print("largest deviations so far: record groups", DEV["rec"], "of their scale, R_acc", DEV["R"], "per entry")


# ------------------------------------------------------------------------------------------------ (b) every refusal and fallback
def path_case(rng, S=80):
    """n = (0.5, 0, 0.5), f = 256 and cx = 80: the pixel x = -176 has n.p = 0 exactly, pixels left of it n.p < 0."""
    nrm, d = np.array([0.5, 0.0, 0.5]), 0.6
    Rprev = K.rotation([0.0, 0.05, 0.0])
    om = np.array([0.002, 0.001, -0.003])
    R = K.rotation(om) @ Rprev
    T = np.array([0.02, -0.01, 0.015])
    key = (rng.uniform(0, 1, (S, 2)) * [160, 128]).astype(np.float32)
    pk = np.concatenate([(key.astype(np.float64) - CXY) / FOC, np.ones((S, 1))], 1)
    q = pk @ R.T
    lam = (d - nrm @ T) / (q @ nrm)
    P = lam[:, None] * q + T
    nxt = (P[:, :2] / P[:, 2:3] * FOC + CXY + rng.normal(0, 0.2, (S, 2))).astype(np.float32)
    key[0] = [80.0 + 256.0 * 40.0, 64.0]                         # rotated behind the camera: Z < min_depth
    nxt[1] = [-176.0, 30.0]                                      # n.p = 0
    nxt[2] = [-400.0, 30.0]                                      # n.p < 0 < n.q: s <= 0
    nxt[3] = [np.nan, 10.0]; nxt[4] = [np.inf, 10.0]; key[5] = [np.nan, np.nan]     # no number in a point
    nxt[6] += 30.0                                               # a wild row: the gate drops it
    st = np.ones(S, np.uint8); st[8] = 0; st[40:44] = 0
    mem = np.ones(S, np.uint8); mem[9] = 0; mem[50:53] = 0
    state = np.zeros(K.KEY_STATE); state[:9] = Rprev.ravel(); state[9:12] = [1.0, 2.0, 3.0]; state[12:15] = [1.1, 2.1, 2.9]
    sn = np.zeros(28); sn[0] = d; sn[1:4] = nrm; sn[4:7] = om; sn[7:16] = K.rotation([0.1, -0.2, 0.3]).ravel(); sn[16:19] = [0.03, -0.02, 0.05]
    sn[19] = 1.0 / FOC; sn[20:22] = CXY
    live = int(np.count_nonzero(st[:S - 2] & mem[:S - 2]))
    return dict(next=nxt, status=st, n=S - 2, sensors=sn, vu=np.array([0.01, -0.02, 0.03]), solved=True, step=11,
                state=dict(key_xy=key, member=mem, state=state, istate=np.array([6, live + 4, 1, 0], np.int32))), live


def test_every_refusal_and_fallback(ctx, ofk):
    rng = np.random.default_rng(11)
    base, live = path_case(rng)
    S = len(base["status"])
    s0 = K.setting(rot_max=0.3)
    nan_om = dict(base, sensors=base["sensors"].copy()); nan_om["sensors"][5] = np.nan
    inf_om = dict(base, sensors=base["sensors"].copy()); inf_om["sensors"][4] = np.inf
    same_pt = dict(base, state=dict(base["state"], key_xy=np.tile(base["state"]["key_xy"][20], (S, 1))), next=np.tile(base["next"][20], (S, 1)))
    nan_off = dict(base, sensors=base["sensors"].copy()); nan_off["sensors"][17] = np.nan
    inf_rw = dict(base, sensors=base["sensors"].copy()); inf_rw["sensors"][9] = np.inf
    variants = [("offset-nan", s0, nan_off), ("rworld-inf", s0, inf_rw), ("default", s0, base), ("gate-0", dict(s0, gate=0.0), base), ("gate-tiny", dict(s0, gate=0.4), base),
                ("omega-nan", s0, nan_om), ("omega-inf", s0, inf_om), ("rank-2", s0, same_pt), ("unsolved-record", s0, dict(nan_om, solved=False)),
                ("vu-nan", s0, dict(nan_om, vu=np.array([0.0, np.nan, 0.0])))]
    seen = {}
    for name, s, case in variants:                               # a launch has one setting: each variant in a launch of its own
        got, rec, want = run_stage(ctx, ofk, [case], s, [3], S)
        compare_stage(got, rec, want, name)
        seen[name] = (want[0][1], want[0][3], got)
    r, dg, _ = seen["default"]
    # one row behind the camera (the NaN key point too), one with n.p = 0 (the NaN next point too), one with s < 0 (the infinite next
    # point too: its s is 0)
    assert dg["no_z"] == 2 and dg["no_den"] == 2 and dg["no_s"] == 2 and r[28] == live and r[4] == live - 6, (dg, r)
    assert r[3] == 0 and r[29] == 1 and r[5] == r[4] - 1 and r[6] < 0.5 and r[9] == 0, r        # the gated solve stands without the wild row
    g0 = seen["gate-0"][0]
    assert g0[3] == 0 and g0[29] == 0 and g0[5] == 0 and g0[6] > r[6], g0                       # one solve; the wild row is in its residual
    gt = seen["gate-tiny"][0]
    assert gt[3] == 0 and gt[29] == 0 and 0 < gt[5] < 8 and np.array_equal(gt[0:3], g0[0:3]), gt      # five rows within 0.4 px of the first solve (the wild row pulls it): the gated solve is refused for min_rows
    for name in ("omega-nan", "omega-inf"):
        o, _, got = seen[name]
        assert o[3] == 1 and o[4] == 0 and o[9] == 1 and int(o[30]) & 1 and o[27] == 1, (name, o)  # nothing solved: dead-reckoned, re-keyed
        assert np.array_equal(got["state"][0, :9], np.eye(3).ravel())                               # ... with R_acc = I again
        assert np.allclose(o[13:16], np.array([1.1, 2.1, 2.9]) + base["vu"])
    for name in ("offset-nan", "rworld-inf"):                    # the sums are finite, D is not: the solve does not stand
        o = seen[name][0]
        assert o[3] == 1 and o[4] == r[4] and o[5] == r[5] and o[29] == 0 and o[9] == 1 and o[27] == 1, (name, o)
        assert not o[0:3].any() and o[6] == 0 and not o[20:26].any(), (name, o)
        assert np.allclose(o[13:16], np.array([1.1, 2.1, 2.9]) + base["vu"]) and np.array_equal(o[16:19], o[13:16]), (name, o)
    k2 = seen["rank-2"][0]
    assert k2[3] == 1 and k2[4] >= 60 and k2[9] == 1, k2
    un = seen["unsolved-record"][0]
    assert un[3] == 1 and np.array_equal(un[13:16], [1.1, 2.1, 2.9]) and un[27] == 1, un          # the position stays
    vn = seen["vu-nan"][0]
    assert np.array_equal(vn[13:16], [1.1, 2.1, 2.9]), vn


def test_python_stage_entries(pkg, ofk):
    """velocity_node.keyframe_step and simulation.keyframe_step: the restatement's rows through the facade, from no state to a keyframe."""
    from of_amd import simulation, velocity_node
    rng = np.random.default_rng(5)
    key, nxt, sn, st0 = scene(rng, S=120)
    for mod in (velocity_node, simulation):
        state, want = None, K.empty(120)
        for t, pts in enumerate((key, nxt)):
            sn_t = sn.copy()
            if t == 0:
                sn_t[4:7] = 0.0
            state, rec = mod.keyframe_step(pts, sn_t, (0.01, 0.02, 0.03), state=state, step=t, rot_max=0.3)
            want, wrec, count, _ = K.step(want, pts, np.ones(120, np.uint8), 120, sn_t, (0.01, 0.02, 0.03), True, t, K.setting(rot_max=0.3))
            assert np.array_equal(state["member"], want["member"][:count]) and np.array_equal(bits(state["key_xy"]), bits(want["key_xy"][:count]))
            same_record(rec, wrec, (mod.__name__, t))
        assert rec[3] == 0 and rec[7] == 120 and rec[8] == 1


# ------------------------------------------------------------------------------------------------ (c)-(f) streams
H, W, NF, B = 128, 160, 9, 2
MOTION = dict(v=(0.012, -0.008, 0.004), omega=(0.002, -0.001, 0.004), d=1.0)
MC, MF, RADIUS = 120, 100, 5
MC_BEGIN = 100                                                   # ofk_stream_step's streams begin with fewer corners than their steps may hold: rows are appended
_frames = {}


def frames_of(pkg, motion="linear"):
    if motion not in _frames:
        from of_amd import synth
        seqs = [synth.render_sequence(H, W, 60 + b, NF, margin=64, motion=motion, **MOTION) for b in range(B)]
        _frames[motion] = (np.stack([s[0] for s in seqs]), seqs[0][1])
    return _frames[motion]


def stream_cfg(**kw):
    from of_amd.pipeline import PipelineConfig
    return PipelineConfig(max_corners=MC, quality=0.01, min_distance=4, block_size=5, win=15, max_level=2, max_count=20, eps=0.03, min_eig_thr=1e-4, **kw)


def sensor_rows(ofk, info, n=B):
    rot = K.rotation([0.02, -0.01, 0.03])
    return ofk.make_sensors(n, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"],
                            v_prior=info["v"], rotation=rot, offset=(0.01, -0.02, 0.1))


class Follower:
    """The restated keyframe state of a context's streams, advanced with what the calls hand back and compared after every call."""

    def __init__(self, ctx, S, s=K.DEFAULTS):
        self.ctx, self.S, self.s = ctx, S, s

    def start(self, counts, step=0):
        """The streams have no keyframe state: the device begins it in front of the next step."""
        self.B = len(counts)
        self.st = [K.empty(self.S) for _ in range(self.B)]
        self.n = [int(c) for c in counts]
        self.rec = [None] * self.B
        self.table_step = [step] * self.B
        return self

    def replaced(self, b, count):
        self.st[b]["member"][:count] = 0; self.st[b]["key_xy"][:count] = 0
        self.st[b]["istate"][1] = 0
        self.n[b] = int(count)
        if self.rec[b] is not None:
            self.rec[b] = None                                   # the record is the previous step's: its members_at_key is stale

    def compare(self, tag):
        d = self.ctx.keyframe_download(self.B, self.S)
        for b in range(self.B):
            n = self.n[b]
            assert np.array_equal(bits(d["key_xy"][b, :n]), bits(self.st[b]["key_xy"][:n])), (tag, b, "key_xy")
            assert np.array_equal(d["member"][b, :n], self.st[b]["member"][:n]), (tag, b, "member")
            w = self.st[b]["state"][:9]
            err = float(np.abs(d["R_acc"][b].ravel() - w).max())
            DEV["R"] = max(DEV["R"], err)
            assert err <= R_TOL, (tag, b, d["R_acc"][b], w)
            if self.rec[b] is not None:
                same_record(d["rec"][b], self.rec[b], (tag, b))
        return d

    def step(self, rec, counts, max_total, sensors, fused, tag, held=False, imu=None, ideal_next=None):
        if held:                                                 # a held step launches nothing (a replace in front of it has happened)
            return self.compare((tag, "held"))
        nxt, keep = self.ctx.stream_last_points(self.S)
        for b in range(self.B):
            n_old = self.n[b]
            pts = nxt[b] if ideal_next is None else ideal_next[b]
            kept = int(np.count_nonzero(keep[b, :n_old]))
            solved = rec[b, 15] != 0 if fused else rec[b, 4] >= 3
            self.st[b], self.rec[b], count, _ = K.step(self.st[b], pts[:self.S], keep[b], n_old, sensors[b], rec[b, 8:11], bool(solved), self.table_step[b],
                                                       self.s, new_count=int(counts[b]) - kept, max_total=max_total,
                                                       imu=None if imu is None else imu[b])
            assert count == counts[b], (tag, b, count, counts[b])
            self.n[b] = int(counts[b]); self.table_step[b] += 1
        d = self.compare(tag)
        for b in range(self.B):                                  # R_acc is compared step by step: the next step starts from the device's
            self.st[b]["state"][:9] = d["R_acc"][b].ravel()
        return d


def jpeg_of(batch):
    from PIL import Image
    res = []
    for img in batch:
        buf = _io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=92)
        res.append(buf.getvalue())
    return res


SET_STREAM = K.setting(min_share=0.9, rot_max=0.02)             # 8 steps of 0.0046 rad: the keyframe is handed over by angle, or by share before


def run_plain(pkg, ofk, keyf, jpeg_step=None, on_from=1):
    """ofk_stream_step over the 8 steps; the streams begin with MC_BEGIN corners and re-detect up to MC whenever they hold fewer; keyf:
    the setting is on (from step on_from on).  jpeg_step: that step's frames arrive as JPEG streams.  -> everything the calls returned."""
    frames, info = frames_of(pkg)
    cfg, sensors = stream_cfg(), sensor_rows(ofk, info)
    ctx = ofk.Context(0, W, H, B, MC, cfg.max_level)
    out, fol, flags, reasons, appended = [], None, [], set(), 0
    try:
        ctx.set_track_table(ofk.track_table_setting())
        tracks, counts = ctx.stream_begin(frames[:, 0], dataclasses.replace(cfg, max_corners=MC_BEGIN).to_params())
        out.append((tracks.copy(), counts.copy()))
        for t in range(1, NF):
            if keyf and t == on_from:
                ctx.set_keyframe(device_setting(ofk, SET_STREAM))
                fol = Follower(ctx, MC, SET_STREAM).start(counts, step=t - 1)
            before = counts.copy()
            if t == jpeg_step:
                rec, tracks, counts = ctx.stream_step_jpeg(jpeg_of(frames[:, t]), sensors, cfg.to_params(), MC, RADIUS)
            else:
                rec, tracks, counts = ctx.stream_step(frames[:, t], sensors, cfg.to_params(), MC, RADIUS)
            out.append((rec.copy(), tracks.copy(), counts.copy(), ctx.track_table_download(B, MC)))
            if fol:
                d = fol.step(rec, counts, MC, sensors, False, ("plain", t))
                flags += [int(f) for f in d["rec"][:, 3]]
                reasons |= {int(r) for r in d["rec"][:, 9]}
                appended += int((counts > before).sum())
                print("plain step", t, "counts", before, "->", counts, "flags", d["rec"][:, 3], "reasons", d["rec"][:, 9], "live", d["rec"][:, 28],
                      "rms px", d["rec"][:, 6], "pos", d["rec"][:, 13:16])
        if fol and on_from == 1 and jpeg_step is None:
            assert flags[:B] == [2] * B and flags.count(0) >= 4 * B and appended >= 1, (flags, appended)
            assert len(reasons - {0, 1}) >= 1, reasons           # a handover that is not the first keying
    finally:
        ctx.close()
    return out


def same(a, b, tag):
    assert len(a) == len(b), tag
    for k, (x, y) in enumerate(zip(a, b)):
        for i, (p, q) in enumerate(zip(x, y)):
            if isinstance(p, dict):
                assert all(np.array_equal(p[key], q[key]) for key in p), (tag, k, i)
            else:
                assert np.array_equal(p.view(np.uint8), q.view(np.uint8)), (tag, k, i)


def test_stream_step_and_on_is_off_for_everything_else(pkg, ofk):
    same(run_plain(pkg, ofk, True), run_plain(pkg, ofk, False), "plain: on against off")


def test_stream_step_jpeg(pkg, ofk):
    pytest.importorskip("PIL.Image")
    run_plain(pkg, ofk, True, jpeg_step=3)


def test_setting_switched_on_in_the_middle_of_a_stream(pkg, ofk):
    run_plain(pkg, ofk, True, on_from=4)


def run_fused(pkg, ofk, keyf, kind):
    """ofk_stream_step_fused on the sensors, no filter.  kind: "robust" (the robust solve drops its outliers from the tracks) | "replace"
    (streams with few tracks replace them in front of LK) | "hold" (one stream; steps 3 and 4 are not solved and held) | "imu" |
    "both" (the depths and the templates on as well: their bits beside the keyframe) | "bias" | any of "camera", "rs" (the rolling shutter
    in flow mode), "rsg" (in gyro mode) and "finite" joined with "+"."""
    from of_amd.pipeline import CameraModel, FusionConfig
    parts = kind.split("+")
    finite = "finite" in parts
    rs_mode = "flow" if "rs" in parts else "gyro" if "rsg" in parts else None
    frames, info = frames_of(pkg, "finite" if finite else "linear")
    nb = 1 if kind == "hold" else B
    frames = frames[:nb]
    robust = kind == "robust"
    cfg = stream_cfg(**(dict(robust="tukey", robust_drop=True) if robust else {}))
    sensors = sensor_rows(ofk, info, nb)
    fusion = FusionConfig(use_imu=kind == "imu", redetect_replace=kind == "replace", hold_on_skip=kind == "hold")
    cam = CameraModel(fx=160.0, fy=160.0, cx=80.0, cy=64.0, k=(-0.1, 0.01, 0, 0)) if "camera" in parts else None
    if cam is not None:
        sensors[:, 19:22] = cam.sensor_slots()
    if kind == "bias":
        sensors[:, 4:7] += [0.001, -0.002, 0.0015]               # a gyro that is off: the setting's estimate is taken out in front of the step
    mf = MC - 10 if kind == "replace" else MF
    ctx = ofk.Context(0, W, H, nb, MC, cfg.max_level)
    out, flags, events, differs, moved = [], [], 0, 0, 0
    try:
        if robust:
            ctx.set_robust(cfg.robust_setting())
        if cam is not None:
            ctx.set_camera(cam.setting())
        if rs_mode:
            ctx.set_rolling_shutter(ofk.rshutter_setting(rs_mode, readout=0.6, anchor=0.4))
        if finite:
            ctx.set_finite_motion(ofk.finite_motion_setting())
        if kind == "bias":
            ctx.set_gyro_bias(ofk.gyro_bias_setting(b0=(0.001, -0.002, 0.0015)))
        ctx.imu_reset(nb)
        ctx.set_track_table(ofk.track_table_setting())
        if kind == "both":
            ctx.set_track_depth(ofk.track_depth_setting()); ctx.set_track_template(ofk.track_template_setting())
        if keyf:
            ctx.set_keyframe(device_setting(ofk, SET_STREAM))
        tracks, counts = ctx.stream_begin(frames[:, 0], cfg.to_params())
        fol = Follower(ctx, MC, SET_STREAM).start(counts) if keyf else None
        for t in range(1, NF):
            fs = fusion.to_struct()
            if kind == "hold" and t in (3, 4):
                fs.min_solve = 10 ** 6                           # more points than there are: not solved
            n_before = None if fol is None else list(fol.n)
            raw_prev = np.zeros((nb, MC, 2), np.float32); raw_prev[:, :tracks.shape[1]] = tracks       # the tracks the step starts from
            rec, fused, tracks, counts = ctx.stream_step_fused(frames[:, t], sensors, cfg.to_params(), fs, mf, RADIUS)
            hold = kind == "hold" and rec[0, 15] == 0
            extra = ()
            if kind == "both":
                extra = (ctx.track_depth_download(nb, MC), {k: v for k, v in ctx.track_template_download(nb, MC).items() if k != "tmpl"})
            out.append((rec.copy(), fused.copy(), tracks.copy(), counts.copy(), ctx.track_table_download(nb, MC)) + extra)
            if fol:
                if kind == "replace":                            # k_redetect_limits' rule: a stream with few tracks and a budget starts over
                    tab = ctx.track_table_download(nb, MC)
                    for b in range(nb):
                        if n_before[b] <= mf and MC - n_before[b] > 0:
                            fol.replaced(b, int(tab["stats"][b, 1] + tab["stats"][b, 2]))    # the rows LK saw: kept + lost
                            events += 1
                imu = ctx.imu_state(nb)[0] if kind == "imu" else None
                sn = sensors
                if kind == "bias":                               # the omega the solve read: the raw one less the setting's estimate (slots 12-14)
                    sn = sensors.copy(); sn[:, 4:7] = ctx.gyro_bias_download(nb)[:, 12:15]
                    assert np.abs(sn[:, 4:7] - sensors[:, 4:7]).max() > 5e-4
                ideal = None
                if (cam is not None or rs_mode or finite) and not hold:
                    # the ideal next points in front of the finite-motion rewrite, rebuilt with the stage entries: the lens undone, then
                    # the rolling shutter's correction, which reads the raw rows and both ends of every point
                    raw, _ = ctx.stream_last_points(MC)
                    ideal, ideal_prev = raw, raw_prev
                    if cam is not None:
                        ideal, ideal_prev = ctx.undistort_points(cam.setting(), raw), ctx.undistort_points(cam.setting(), raw_prev)
                    if rs_mode:
                        rs = ofk.rshutter_setting(rs_mode, readout=0.6, anchor=0.4, rows=H)
                        _, corrected = ctx.rs_correct_points(rs, raw_prev, raw, counts=n_before, sensors=sensors,
                                                             ideal_prev=None if cam is None else ideal_prev, ideal_next=None if cam is None else ideal)
                        moved += int(np.any(corrected[0, :n_before[0]] != ideal[0, :n_before[0]]))
                        ideal = corrected
                    seen = (ctx.finite_download(nb) if finite else ctx.rs_download(nb) if rs_mode else ctx.camera_download(nb))[1][:, :MC]
                    if finite:
                        differs += int(np.any(seen[0, :n_before[0]] != ideal[0, :n_before[0]]))     # what the solve read is the rewritten point, not this one
                    else:
                        assert all(np.array_equal(bits(seen[b, :n_before[b]]), bits(ideal[b, :n_before[b]])) for b in range(nb))
                d = fol.step(rec, counts, MC, sn, True, (kind, t), held=hold, imu=imu, ideal_next=ideal)
                flags += [int(f) for f in d["rec"][:, 3]]
                events += int(hold)
                if robust:
                    events += int(sum(rec[b, 13] - (rec[b, 11]) for b in range(nb)))       # tracked by LK, not kept by the solve
                print(kind, "step", t, "flags", d["rec"][:, 3], "reasons", d["rec"][:, 9], "live", d["rec"][:, 28], "rms px", d["rec"][:, 6])
        if fol:
            assert flags.count(0) >= (2 if kind in ("replace", "hold") else 4 * nb), (kind, flags)
            if kind in ("robust", "replace", "hold"):            # the case is the one it is named after
                assert events >= (2 if kind == "hold" else 1), (kind, events)
            if finite:
                assert differs >= NF - 2, (kind, differs)        # the rewrite moved the points the solve read; the key solve read the others
            if rs_mode:
                assert moved >= NF - 2, (kind, moved)            # the rolling shutter's correction is in the points the key solve read
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("kind", ["robust", "both"])
def test_stream_step_fused_on_against_off(pkg, ofk, kind):
    same(run_fused(pkg, ofk, True, kind), run_fused(pkg, ofk, False, kind), (kind, "on against off"))


def test_stream_replace_redetection(pkg, ofk):
    run_fused(pkg, ofk, True, "replace")


def test_held_steps_leave_the_keyframe(pkg, ofk):
    run_fused(pkg, ofk, True, "hold")


@pytest.mark.parametrize("kind", ["imu", "camera", "finite", "camera+finite", "rs", "rsg", "rs+finite", "rsg+finite", "camera+rs+finite",
                                  "camera+rsg+finite", "bias"])
def test_composition(pkg, ofk, kind):
    run_fused(pkg, ofk, True, kind)


def test_refusals_download_and_reset(pkg, ofk):
    from of_amd.pipeline import FusionConfig
    frames, info = frames_of(pkg)
    cfg, sensors = stream_cfg(), sensor_rows(ofk, info)
    ctx = ofk.Context(0, W, H, B, MC, cfg.max_level)
    try:
        ctx.imu_reset(B)
        ctx.set_keyframe(ofk.keyframe_setting())
        tracks, counts = ctx.stream_begin(frames[:, 0], cfg.to_params())
        plain = FusionConfig(use_imu=False).to_struct()
        for call in (lambda: ctx.stream_step(frames[:, 1], sensors, cfg.to_params(), MF, RADIUS),
                     lambda: ctx.stream_step_fused(frames[:, 1], sensors, cfg.to_params(), plain, MF, RADIUS)):
            with pytest.raises(ofk.OfkError) as e:               # the track table is off
                call()
            assert e.value.code == ofk.E_INVALID and "ofk_set_track_table" in str(e.value)
        ctx.set_track_table(ofk.track_table_setting())
        legacy = FusionConfig(use_imu=False, keep=ofk.KEEP_LEGACY)
        cases = [(dataclasses.replace(cfg, solve_variant=ofk.SOLVE_OFMODULE), legacy), (cfg, FusionConfig(use_imu=False, flow=ofk.FLOW_ROTATIONAL)), (cfg, legacy)]
        for c, f in cases:
            with pytest.raises(ofk.OfkError) as e:
                ctx.stream_step_fused(frames[:, 1], sensors, c.to_params(), f.to_struct(), MF, RADIUS)
            assert e.value.code == ofk.E_INVALID and "ofk_set_keyframe" in str(e.value), str(e.value)
        with pytest.raises(ofk.OfkError):                          # nothing was launched: no state yet
            ctx.keyframe_download(B)
        with pytest.raises(ofk.OfkError):
            ctx.keyframe_reset(B, [0.0, 0.0, 0.0])
        with pytest.raises(ofk.OfkError):
            ctx.keyframe_reset(0, [0.0, np.nan, 0.0])
        ctx.keyframe_reset(1, [5.0, 6.0, 7.0])                   # before any step: the state begins, stream 1 at the given position
        d = ctx.keyframe_download(B, MC)
        assert np.array_equal(d["rec"][:, 13:16], [[0, 0, 0], [5, 6, 7]]) and np.array_equal(d["rec"][:, 3], [2, 2]) and not d["member"].any()
        assert np.array_equal(d["R_acc"], np.stack([np.eye(3)] * B))
        fol = Follower(ctx, MC).start(counts)
        fol.st[1]["state"][9:15] = [5, 6, 7, 5, 6, 7]
        rec, fused, tracks, counts = ctx.stream_step_fused(frames[:, 1], sensors, cfg.to_params(), plain, MF, RADIUS)     # the stream goes on
        d = fol.step(rec, counts, MC, sensors, True, "after reset")
        assert np.array_equal(d["rec"][:, 3], [2, 2]) and np.array_equal(d["rec"][:, 27], [1, 1]) and np.array_equal(d["rec"][:, 26], [1, 1])
        assert np.allclose(d["rec"][1, 13:16], np.array([5.0, 6.0, 7.0]) + rec[1, 8:11]) and rec[:, 15].all()
        rec, fused, tracks, counts = ctx.stream_step_fused(frames[:, 2], sensors, cfg.to_params(), plain, MF, RADIUS)
        d = fol.step(rec, counts, MC, sensors, True, "second step")
        assert np.array_equal(d["rec"][:, 3], [0, 0])
        ctx.keyframe_reset(0, None)                              # in mid-stream: the members go, the position is loaded
        fol.st[0]["member"][:] = 0; fol.st[0]["istate"][1] = 0; fol.st[0]["state"][:] = K.empty(1)["state"]; fol.rec[0] = None
        d = fol.compare("reset in mid-stream")
        want = np.zeros(K.KEY_DOUBLES); want[3] = 2; want[8] = fol.st[0]["istate"][0]; want[26] = fol.st[0]["istate"][2]; want[27] = fol.st[0]["istate"][3]
        assert np.array_equal(d["rec"][0], want), d["rec"][0]    # nothing of the last step's solve stays beside flag 2
        rec, fused, tracks, counts = ctx.stream_step_fused(frames[:, 3], sensors, cfg.to_params(), plain, MF, RADIUS)
        d = fol.step(rec, counts, MC, sensors, True, "third step")
        assert np.array_equal(d["rec"][:, 3], [2, 0])
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ (g) a sequence through FlowStream
def test_finite_motion_sequence_through_flowstream_with_templates(pkg, ofk):
    """12 frames of 240 x 320 rendered with the exact motion of every step, through FlowStream with the track table, the templates,
    finite motion and the keyframe on, no re-detection.  The CPU run of the same frames (keyframe_reference.rendered: the C oracle's LK,
    the template restatement, the keyframe restatement) ends 4.27e-4 d from the truth (measured; its summed step solves 1.28e-3); the
    device's position must lie within twice that (measured: 4.38e-4)."""
    from of_amd.pipeline import FlowStream, PipelineConfig
    nf, size = 12, dict(h=240, w=320, corners=150)
    cpu = K.rendered(True, nf, **size)
    seq = K.rendered_sequence(nf, **size)
    cfg = PipelineConfig(max_corners=150, quality=0.01, min_distance=10, block_size=3, win=15, max_level=3, max_count=30, eps=0.01, min_eig_thr=1e-4,
                         track_table=True, track_template=True, finite_motion=True, keyframe=True)
    fs = FlowStream(320, 240, batch=1, cfg=cfg, min_features=0, mask_radius=5)
    try:
        fs.begin(seq["bgr"][None, 0])
        for j in range(1, nf):
            fs.step(seq["bgr"][None, j], K.rendered_sensors(seq, j)[None])
            p = fs.position()
        err = float(np.linalg.norm(p["pos"][0] - seq["truth"][nf - 1]) / seq["info"]["d"])
        print("position error / d at step", nf - 1, ": device", err, "CPU chain", cpu["key"], "summed step solves on the CPU", cpu["dr"],
              "flag", p["flag"], "live", p["live"], "keyframes", p["keyframes"], "members", len(p["ids"][0]))
        assert p["flag"][0] == ofk.KEY_SOLVED and p["keyframes"][0] >= 1 and p["dead_reckoned"][0] == 1
        assert len(p["ids"][0]) == p["live"][0] or p["reason"][0] != 0          # the members' ids come from the table
        assert abs(cpu["key"] - 4.27e-4) < 0.5e-4                # the figure of the docstring is the CPU run's
        assert err <= 2.0 * cpu["key"], (err, cpu["key"])
    finally:
        fs.close()
