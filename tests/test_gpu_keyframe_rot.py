"""GPU: the keyframe's rotation refined from the flow (include/ofk.h: ofk_set_keyframe_rotation) against its restatement
(tests/keyframe_rot_reference.py), on the shapes of tests/test_gpu_keyframe.py.

(a) ofk_keyframe_rotation_step at the kernel's edges: test_gpu_keyframe's counts, status and member patterns and appends, an error of
    1e-3 rad put into the R_acc the step starts from, both sources (the attitude source with a valid R_world(key), and with none: it
    then runs as source gyro), one axis held, iters 1 and 2.  Flags, counts, iterations, key_xy, member, the re-key reasons, the
    rotation state agree bit for bit; T, delta, pos, C_T, C_delta, R^ within 1e-9 of their group's scale (the keyframe test's bound).
    The largest deviations met are kept in DEV and printed (-s) for the README.
(b) every axis held: state and record are ofk_keyframe_step's on the same inputs, bit for bit.
(c) three streams of different counts; a batch past 64 streams against the same streams in small launches.
(d) ofk_stream_step, ofk_stream_step_fused (plain and robust), a JPEG step, held steps, the replace re-detection and
    ofk_keyframe_reset with the setting on: after every call the downloaded keyframe state, record and rotation record are the bits
    of the stage entries chained on what the calls handed back (the same kernel on the same inputs), and everything else a step
    returns is bit-identical to the keyframe alone.  Nothing of the keyframe is fed back, so a re-key at another step changes none of
    it.  Off after on equals a context that never saw the setting.
(e) refusals, download before any step, the getter's round trip.
(f) the 12-frame finite-motion sequence through FlowStream with a gyro error of 1e-3 rad per frame in the sensors' omega."""
import numpy as np
import pytest

import keyframe_reference as K
import keyframe_rot_reference as RR
import test_gpu_keyframe as G
from test_gpu_keyframe import bits

pytestmark = pytest.mark.gpu
DEV = dict(rec=0.0, rrec=0.0)                                    # the largest deviations met, in units of the group's scale
REC_TOL = 1e-9
R_EXACT = [3, 31, 35, 36, 37, 38, 39]
R_GROUPS = ((0, 3), (4, 13), (13, 19), (19, 25), (25, 28), (28, 31), (32, 35))


def device_rot(ofk, r):
    return ofk.keyframe_rotation_setting(True, r["source"], r["axes"], r["sigma_gyro"], r["sigma_bias"], r["sigma_att"], r["iters"], r["delta_max"])


def same_rrec(got, want, tag):
    assert np.array_equal(bits(got[R_EXACT]), bits(want[R_EXACT])), (tag, got, want)
    for lo, hi in R_GROUPS:
        if np.all(np.isfinite(want[lo:hi])):
            scale = max(np.abs(want[lo:hi]).max(), 1e-300)
            err = float((np.abs(got[lo:hi] - want[lo:hi]) / scale).max())
            DEV["rrec"] = max(DEV["rrec"], err)
            assert err <= REC_TOL, (tag, lo, got[lo:hi], want[lo:hi])
        else:
            assert np.array_equal(bits(got[lo:hi]), bits(want[lo:hi])), (tag, lo, got[lo:hi], want[lo:hi])


@pytest.fixture(scope="module")
def ctx(ofk):
    c = ofk.Context(0, 64, 48, 70, 1100, 2)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ (a)-(c) the stage entry
def rot_case(rng, n, pattern, mpattern, b, variant, att):
    """test_gpu_keyframe's edge case with 1e-3 rad of error in its R_acc and a rotation state: valid for the attitude source on even b."""
    c = G.edge_case(rng, n, pattern, mpattern, b, variant)
    st, sn = c["state"], c["sensors"]
    Rtrue_prev = st["state"][:9].reshape(3, 3)
    err = K.rotation(rng.normal(0, 1e-3, 3))
    st["state"][:9] = (err @ Rtrue_prev).ravel()
    rs = np.zeros(RR.ROT_STATE)
    if att and b % 2 == 0:                                       # R_world(key) such that R_world(now)^T R_world(key) is the erring R_acc
        Rw = sn[7:16].reshape(3, 3)
        rs[:9] = (Rw @ (err @ (K.rotation(sn[4:7]) @ Rtrue_prev))).ravel(); rs[9] = 1.0; rs[10] = float(st["istate"][0])
    else:
        rs[:9] = rng.normal(0, 1, 9); rs[9] = float(b % 3 == 1); rs[10] = float(st["istate"][0] + 1)     # stale: not this keyframe's
    st["rstate"] = rs
    return c


def run_rot_stage(ctx, ofk, cases, s, r, new_counts, max_total):
    st = {k: np.stack([c["state"][k] for c in cases]) for k in ("key_xy", "member", "state", "istate", "rstate")}
    got, rec, rrec = ctx.keyframe_rotation_step(
        np.stack([c["next"] for c in cases]), np.stack([c["status"] for c in cases]), [c["n"] for c in cases],
        np.stack([c["sensors"] for c in cases]), np.stack([c["vu"] for c in cases]), [int(c["solved"]) for c in cases], [c["step"] for c in cases],
        st, new_counts=new_counts, max_total=max_total, keyframe=G.device_setting(ofk, s), rotation=device_rot(ofk, r))
    want = [RR.step(c["state"], c["next"], c["status"], c["n"], c["sensors"], c["vu"], c["solved"], c["step"], s, r,
                    None if new_counts is None else new_counts[b], max_total) for b, c in enumerate(cases)]
    return got, rec, rrec, want


def compare_rot_stage(got, rec, rrec, want, tag):
    theirs = dict(G.DEV)                                         # test_gpu_keyframe's own tally stays its own
    G.DEV["rec"] = 0.0
    for b, (wst, wrec, wrrec, count, _) in enumerate(want):
        assert np.array_equal(bits(got["key_xy"][b, :count]), bits(wst["key_xy"][:count])), (tag, b, "key_xy")
        assert np.array_equal(got["member"][b, :count], wst["member"][:count]), (tag, b, "member")
        G.same_state(got["state"][b], got["istate"][b], wst, (tag, b))
        G.same_record(rec[b], wrec, (tag, b))
        same_rrec(rrec[b], wrrec, (tag, b))
        assert np.array_equal(bits(got["rstate"][b]), bits(wst["rstate"])), (tag, b, "rstate", got["rstate"][b], wst["rstate"])
    DEV["rec"] = max(DEV["rec"], G.DEV["rec"])
    G.DEV.update(theirs)


def check_rot(ctx, ofk, ns, pattern, mpattern, appended, case, s, r):
    import zlib
    rng = np.random.default_rng(zlib.crc32(repr((tuple(ns), pattern, mpattern, appended, "rot")).encode()))
    att = r["source"] == RR.ATTITUDE
    cases = [rot_case(rng, n, pattern, mpattern, b, b + len(appended) + len(pattern), att) for b, n in enumerate(ns)]
    kept = [int(np.count_nonzero(c["status"][:c["n"]])) for c in cases]
    if appended == "none":
        new_counts, max_total = None, G.S_EDGE
    elif appended == "some":
        new_counts, max_total = [17 + b for b in range(len(ns))], G.S_EDGE
    else:
        new_counts, max_total = [40] * len(ns), min(G.S_EDGE, max(kept) + 5)
    got, rec, rrec, want = run_rot_stage(ctx, ofk, cases, s, r, new_counts, max_total)
    compare_rot_stage(got, rec, rrec, want, (case, tuple(ns), max_total))
    return [w[2] for w in want], [w[1] for w in want]


ROTS = (RR.setting(sigma_bias=3e-4), RR.setting(source="attitude", sigma_att=1e-3, sigma_bias=3e-4),
        RR.setting(sigma_bias=3e-4, axes=(1, 0, 1), iters=1), RR.setting(source="attitude", sigma_att=1e-3, sigma_bias=0.0, sigma_gyro=2e-4, iters=1))


@pytest.mark.parametrize("pattern", G.PATTERNS)
def test_rot_step_kernel_edges(ctx, ofk, pattern):
    groups = [G.COUNTS[0:3], G.COUNTS[3:6], G.COUNTS[6:9], (G.COUNTS[9], G.COUNTS[4], G.COUNTS[7])]
    flags, sources, deltas = [], [], []
    for m, mpattern in enumerate(G.PATTERNS):
        for g, ns in enumerate(groups):
            s = dict(G.SET, max_age=(0, 4, 40)[(g + m) % 3])
            rr, recs = check_rot(ctx, ofk, ns, pattern, mpattern, ("none", "some", "clamped")[(g + m) % 3], (pattern, mpattern, g), s, ROTS[(g + 2 * m) % 4])
            flags += [int(q[3]) for q in rr]; sources += [int(q[35]) for q in rr if q[3] == RR.OK]
            deltas += [float(np.abs(q[0:3]).max()) for q in rr if q[3] == RR.OK]
    if pattern in ("all", "random"):
        assert flags.count(RR.OK) >= 6 and RR.NONE in flags, flags           # the comparison of delta and C_delta is not one of zeros
        assert 0 in sources and 1 in sources, sources
        assert max(deltas) > 2e-4, deltas                                   # the error put into R_acc is found
    print("largest deviations so far: keyframe record", DEV["rec"], "rotation record", DEV["rrec"], "of their groups' scale")


def test_rot_all_axes_held_is_the_plain_step(ctx, ofk):
    rng = np.random.default_rng(11)
    cases = [rot_case(rng, n, "random", "all", b, 0, False) for b, n in enumerate((513, 64, 257))]
    st = {k: np.stack([c["state"][k] for c in cases]) for k in ("key_xy", "member", "state", "istate", "rstate")}
    args = (np.stack([c["next"] for c in cases]), np.stack([c["status"] for c in cases]), [c["n"] for c in cases],
            np.stack([c["sensors"] for c in cases]), np.stack([c["vu"] for c in cases]), [int(c["solved"]) for c in cases], [c["step"] for c in cases])
    kf = G.device_setting(ofk, G.SET)
    want, wrec = ctx.keyframe_step(*args, st, new_counts=[5, 6, 7], max_total=G.S_EDGE, keyframe=kf)
    assert (wrec[:, 3] == 0).any()
    for r in (RR.setting(axes=(0, 0, 0)), RR.setting(sigma_bias=0.0, sigma_gyro=0.0), RR.setting(source="attitude", sigma_att=0.0)):
        got, rec, rrec = ctx.keyframe_rotation_step(*args, st, new_counts=[5, 6, 7], max_total=G.S_EDGE, keyframe=kf, rotation=device_rot(ofk, r))
        for k in ("key_xy", "member", "state", "istate"):
            assert np.array_equal(bits(got[k]), bits(want[k])), (r, k)
        assert np.array_equal(bits(rec), bits(wrec)), r
        assert np.array_equal(bits(got["rstate"]), bits(st["rstate"])), r
        want_rrec = np.zeros((3, RR.ROT_DOUBLES)); want_rrec[:, 3] = RR.HELD
        assert np.array_equal(bits(rrec), bits(want_rrec)), r


def fallback_cases():
    """test_gpu_keyframe's path case (rows behind the camera, with n.p = 0, without a number, a wild row) with 1e-2 rad of error in its
    R_acc, per variant (name, keyframe setting, rotation setting, case, the rotation's flag).  age = 6."""
    rng = np.random.default_rng(11)
    base, live = G.path_case(rng)
    S = len(base["status"])
    st = dict(base["state"], state=base["state"]["state"].copy(), rstate=np.zeros(RR.ROT_STATE))
    st["state"][:9] = (K.rotation([6e-3, -5e-3, 6e-3]) @ st["state"][:9].reshape(3, 3)).ravel()
    base = dict(base, state=st)
    s0, r0 = K.setting(rot_max=0.3), RR.setting(sigma_bias=5e-3)
    nan_off = dict(base, sensors=base["sensors"].copy()); nan_off["sensors"][17] = np.nan
    inf_rw = dict(base, sensors=base["sensors"].copy()); inf_rw["sensors"][9] = np.inf
    two = np.arange(S) % 2                                       # two points, forty times each: T is determined, (T, delta) is not
    pair = dict(base, state=dict(st, key_xy=st["key_xy"][[20, 21]][two]), next=base["next"][[20, 21]][two])
    return [("default", s0, r0, base, RR.OK), ("gate-0", dict(s0, gate=0.0), r0, base, RR.OK), ("gate-tiny", dict(s0, gate=0.05), r0, base, RR.OK),
            ("large", s0, RR.setting(sigma_bias=5e-3, delta_max=2e-3), base, RR.LARGE), ("large gate-0", dict(s0, gate=0.0), RR.setting(sigma_bias=5e-3, delta_max=2e-3), base, RR.LARGE),
            ("singular", s0, RR.setting(sigma_bias=np.inf), pair, RR.SINGULAR), ("two points with a prior", s0, r0, pair, RR.OK),
            ("offset-nan", s0, r0, nan_off, RR.NONE), ("rworld-inf", s0, r0, inf_rw, RR.NONE)]


def test_rot_every_fallback_leaves_the_plain_step(ctx, ofk):
    """Every way the joint rule gives way, on the device: |delta^| > delta_max, a reduced system that is not positive, a displacement
    that is no number behind a joint solve that stood (NaN lever arm, infinite R_world), and the joint rule with gate 0 and with a gate
    that leaves too few rows.  Where the rotation's flag is not OK, key_xy, member, state, istate and the keyframe's record are
    ofk_keyframe_step's on the same inputs bit for bit; everything is compared with the restatement as well."""
    seen = {}
    for name, s, r, case, flag in fallback_cases():              # a launch has one setting: each variant in a launch of its own
        S = len(case["status"])
        got, rec, rrec, want = run_rot_stage(ctx, ofk, [case], s, r, [3], S)
        compare_rot_stage(got, rec, rrec, want, name)
        assert rrec[0, 3] == flag, (name, rrec[0])
        st = {k: case["state"][k][None] for k in ("key_xy", "member", "state", "istate")}
        pgot, prec = ctx.keyframe_step(case["next"][None], case["status"][None], [case["n"]], case["sensors"][None], case["vu"][None],
                                       [int(case["solved"])], [case["step"]], st, new_counts=[3], max_total=S, keyframe=G.device_setting(ofk, s))
        if flag != RR.OK:
            for k in ("key_xy", "member", "state", "istate"):
                assert np.array_equal(bits(got[k]), bits(pgot[k])), (name, k)
            assert np.array_equal(bits(rec), bits(prec)), (name, rec, prec)
            assert not rrec[0, 13:19].any() and rrec[0, 31] == 0
        seen[name] = (rec[0], rrec[0], prec[0])
    d, q, p = seen["default"]
    assert d[3] == 0 and d[29] == 1 and q[31] == 2 and d[6] < 0.5 * p[6] and np.linalg.norm(q[0:3]) > 5e-3, (d, q, p)   # the error is found; the residual falls
    g0 = seen["gate-0"][0]
    assert g0[3] == 0 and g0[29] == 0 and g0[5] == 0 and g0[6] > d[6], g0                       # one joint solve; the wild row is in its residual
    gt = seen["gate-tiny"][0]
    assert gt[3] == 0 and gt[29] == 0 and gt[5] < 8 and np.array_equal(gt[0:3], g0[0:3]), gt      # fewer than min_rows within 0.05 px: the first joint solve stands
    lg = seen["large"][1]
    assert np.linalg.norm(lg[0:3]) > 2e-3 and seen["large"][0][3] == 0 and seen["large"][0][29] == 1, lg     # refused and reported; the plain gated solve stands
    for name in ("offset-nan", "rworld-inf"):                    # the joint solve stood and is withdrawn: the plain step's bits, its angle R_acc's
        o, q, p = seen[name]
        assert o[3] == 1 and o[5] == p[5] and o[19] == p[19] and not q[0:3].any() and not q[32:35].any(), (name, o, q)
    assert seen["singular"][0][3] == 0 and not seen["singular"][1][25:28].any()


def test_rot_three_streams_of_different_counts(ctx, ofk):
    for k, ns in enumerate(((1030, 0, 257), (1, 513, 64), (300, 300, 299))):
        rr, _ = check_rot(ctx, ofk, ns, "random", "all", "clamped", ("mixed", ns), G.SET, ROTS[k % 2])
        assert sum(q[3] == RR.OK for q in rr) >= 1, ns
    print("largest deviations so far: keyframe record", DEV["rec"], "rotation record", DEV["rrec"], "of their groups' scale")


def test_rot_batch_past_64_streams(ctx, ofk):
    rng = np.random.default_rng(5)
    nb = 70
    cases = [rot_case(rng, (300, 65, 257, 40)[b % 4], "random", "all", b, 0, b % 4 == 2) for b in range(nb)]
    r = device_rot(ofk, ROTS[1]); kf = G.device_setting(ofk, G.SET)

    def run(sel):
        cs = [cases[b] for b in sel]
        st = {k: np.stack([c["state"][k] for c in cs]) for k in ("key_xy", "member", "state", "istate", "rstate")}
        return ctx.keyframe_rotation_step(np.stack([c["next"] for c in cs]), np.stack([c["status"] for c in cs]), [c["n"] for c in cs],
                                          np.stack([c["sensors"] for c in cs]), np.stack([c["vu"] for c in cs]), [int(c["solved"]) for c in cs],
                                          [c["step"] for c in cs], st, new_counts=[3] * len(cs), max_total=G.S_EDGE, keyframe=kf, rotation=r)
    got, rec, rrec = run(range(nb))
    assert (rrec[:, 3] == RR.OK).sum() >= nb // 2 and (rrec[:, 35] == 1).any() and (rrec[64:, 3] == RR.OK).any()
    for sel in ((0, 1, 2), (63, 64, 65), (67, 68, 69)):
        g2, r2, q2 = run(sel)
        idx = list(sel)
        for k in g2:
            assert np.array_equal(bits(got[k][idx]), bits(g2[k])), (sel, k)
        assert np.array_equal(bits(rec[idx]), bits(r2)) and np.array_equal(bits(rrec[idx]), bits(q2)), sel


# ------------------------------------------------------------------------------------------------ (d) streams
ROT_STREAM = RR.setting(sigma_bias=1e-3)


class Chain:
    """The stage entries chained on what the stream's calls hand back; after every call the stream's downloads must be its bits."""

    def __init__(self, ctx, ofk, S, nb):
        self.ctx, self.S, self.nb = ctx, S, nb
        self.kf, self.rot = G.device_setting(ofk, G.SET_STREAM), device_rot(ofk, ROT_STREAM)
        self.st = {k: np.stack([RR.empty(S)[k]] * nb) for k in ("key_xy", "member", "state", "istate", "rstate")}
        self.rec = self.rrec = None
        self.step_no = np.zeros(nb, np.int32)
        self.flags = []

    def start(self, counts):
        self.n = [int(c) for c in counts]
        return self

    def replaced(self, b, count):
        self.st["member"][b, :] = 0; self.st["key_xy"][b, :] = 0; self.st["istate"][b, 1] = 0; self.st["rstate"][b] = 0.0
        self.n[b] = int(count)
        if self.rrec is not None:
            self.rrec[b] = 0.0; self.rrec[b, 3] = RR.NONE

    def step(self, rec, counts, sensors, fused, tag):
        nxt, keep = self.ctx.stream_last_points(self.S)
        kept = [int(np.count_nonzero(keep[b, :self.n[b]])) for b in range(self.nb)]
        solved = [int(rec[b, 15] != 0 if fused else rec[b, 4] >= 3) for b in range(self.nb)]
        self.st, self.rec, self.rrec = self.ctx.keyframe_rotation_step(
            nxt, keep, self.n, sensors, rec[:, 8:11], solved, self.step_no, self.st, new_counts=[int(counts[b]) - kept[b] for b in range(self.nb)],
            max_total=self.S, keyframe=self.kf, rotation=self.rot)
        self.n = [int(c) for c in counts]; self.step_no = self.step_no + 1
        self.flags += [int(f) for f in self.rrec[:, 3]]
        self.compare(tag)

    def compare(self, tag, records=True):
        d = self.ctx.keyframe_download(self.nb, self.S)
        for b in range(self.nb):
            n = self.n[b]
            assert np.array_equal(bits(d["key_xy"][b, :n]), bits(self.st["key_xy"][b, :n])), (tag, b, "key_xy")
            assert np.array_equal(d["member"][b, :n], self.st["member"][b, :n]), (tag, b, "member")
        assert np.array_equal(bits(d["R_acc"].reshape(self.nb, 9)), bits(self.st["state"][:, :9])), (tag, "R_acc")
        if records and self.rec is not None:
            assert np.array_equal(bits(d["rec"]), bits(self.rec)), (tag, "rec", d["rec"], self.rec)
        if self.rrec is not None:
            q = self.ctx.keyframe_rotation_download(self.nb)
            assert np.array_equal(bits(q), bits(self.rrec)), (tag, "rrec", q, self.rrec)
        return d


def run_stream(pkg, ofk, kind, rot):
    """kind: "plain" (ofk_stream_step, append re-detection) | "jpeg" (step 3 as JPEG) | "fused" | "robust" | "hold" | "replace" (as
    test_gpu_keyframe.run_fused).  rot: the rotation on beside the keyframe.  -> everything the calls returned but the keyframe's own."""
    import dataclasses
    from of_amd.pipeline import FusionConfig
    frames, info = G.frames_of(pkg)
    nb = 1 if kind == "hold" else G.B
    frames = frames[:nb]
    fused = kind not in ("plain", "jpeg")
    cfg = G.stream_cfg(**(dict(robust="tukey", robust_drop=True) if kind == "robust" else {}))
    sensors = G.sensor_rows(ofk, info, nb)
    sensors[:, 4:7] += [1e-3, -5e-4, 8e-4]                       # a gyro that is off: there is something to refine
    fusion = FusionConfig(use_imu=False, redetect_replace=kind == "replace", hold_on_skip=kind == "hold")
    mf = G.MC - 10 if kind == "replace" else G.MC if not fused else G.MF
    ctx = ofk.Context(0, G.W, G.H, nb, G.MC, cfg.max_level)
    out, held, events = [], 0, 0
    try:
        if kind == "robust":
            ctx.set_robust(cfg.robust_setting())
        ctx.imu_reset(nb)
        ctx.set_track_table(ofk.track_table_setting())
        ctx.set_keyframe(G.device_setting(ofk, G.SET_STREAM))
        if rot:
            ctx.set_keyframe_rotation(device_rot(ofk, ROT_STREAM))
        tracks, counts = ctx.stream_begin(frames[:, 0], (cfg if fused else dataclasses.replace(cfg, max_corners=G.MC_BEGIN)).to_params())
        chain = Chain(ctx, ofk, G.MC, nb).start(counts) if rot else None
        for t in range(1, G.NF):
            fs = fusion.to_struct()
            if kind == "hold" and t in (3, 4):
                fs.min_solve = 10 ** 6
            n_before = None if chain is None else list(chain.n)
            if kind == "jpeg" and t == 3:
                rec, tracks, counts = ctx.stream_step_jpeg(G.jpeg_of(frames[:, t]), sensors, cfg.to_params(), mf, G.RADIUS)
                fz = None
            elif not fused:
                rec, tracks, counts = ctx.stream_step(frames[:, t], sensors, cfg.to_params(), mf, G.RADIUS)
                fz = None
            else:
                rec, fz, tracks, counts = ctx.stream_step_fused(frames[:, t], sensors, cfg.to_params(), fs, mf, G.RADIUS)
            hold = kind == "hold" and rec[0, 15] == 0
            out.append((rec.copy(), tracks.copy(), counts.copy(), ctx.track_table_download(nb, G.MC)) + (() if fz is None else (fz.copy(),)))
            if chain:
                if kind == "replace":
                    tab = ctx.track_table_download(nb, G.MC)
                    for b in range(nb):
                        if n_before[b] <= mf and G.MC - n_before[b] > 0:
                            chain.replaced(b, int(tab["stats"][b, 1] + tab["stats"][b, 2]))
                            events += 1
                if hold:
                    held += 1
                    chain.compare((kind, t, "held"))             # a held step launches nothing: state and both records stay
                else:
                    chain.step(rec, counts, sensors, fused, (kind, t))
        if rot:
            assert chain.flags.count(RR.OK) >= (2 if kind in ("replace", "hold") else 3 * nb), (kind, chain.flags)
            assert kind != "hold" or held >= 2
            assert kind != "replace" or events >= 1
            if kind == "fused":                                  # ofk_keyframe_reset clears the stream's rotation state too
                ctx.keyframe_reset(0, [1.0, 2.0, 3.0])
                q = ctx.keyframe_rotation_download(nb)
                want = np.zeros(RR.ROT_DOUBLES); want[3] = RR.NONE
                assert np.array_equal(bits(q[0]), bits(want)) and q[1, 3] == chain.rrec[1, 3]
                chain.st["member"][0, :] = 0; chain.st["istate"][0, 1] = 0; chain.st["state"][0] = K.empty(1)["state"]
                chain.st["state"][0, 9:15] = [1, 2, 3, 1, 2, 3]; chain.st["rstate"][0] = 0.0; chain.rrec[0] = want
                chain.compare("reset", records=False)
                rec, fz, tracks, counts = ctx.stream_step_fused(frames[:, 1], sensors, cfg.to_params(), fusion.to_struct(), mf, G.RADIUS)
                chain.step(rec, counts, sensors, True, "after reset")
                assert chain.rrec[0, 3] == RR.NONE and chain.rec[0, 3] == K.NONE
        keyd = ctx.keyframe_download(nb, G.MC)
    finally:
        ctx.close()
    return out, keyd


@pytest.mark.parametrize("kind", ["plain", "fused", "robust"])
def test_rot_stream_steps_compose_and_change_nothing_else(pkg, ofk, kind):
    on, _ = run_stream(pkg, ofk, kind, True)
    off, _ = run_stream(pkg, ofk, kind, False)
    G.same(on, off, (kind, "rotation on against keyframe alone"))


def test_rot_stream_step_jpeg(pkg, ofk):
    pytest.importorskip("PIL.Image")
    run_stream(pkg, ofk, "jpeg", True)


def test_rot_held_steps_and_replace(pkg, ofk):
    run_stream(pkg, ofk, "hold", True)
    run_stream(pkg, ofk, "replace", True)


def test_rot_off_after_on_is_a_context_that_never_saw_it(pkg, ofk):
    """Steps 1-3 with the rotation on, then off in mid-stream, against a context that never saw the setting.  From the switch on every
    step returns the same bits, and the keyframe's state and record are the same bits but for what carries the earlier joint solves'
    positions: pos and anchor (state 9-14, record 13-18).  D, T, C_T, R_acc, key_xy, member and every count are compared.  The sensors'
    omega is exact here, so R^ is R_acc to 1e-4 rad and the re-keys by angle fall on the same steps in both (asserted: key_step)."""
    frames, info = G.frames_of(pkg)
    cfg, sensors = G.stream_cfg(), G.sensor_rows(ofk, info)

    def run(seen):
        ctx = ofk.Context(0, G.W, G.H, G.B, G.MC, cfg.max_level)
        res = []
        try:
            ctx.set_track_table(ofk.track_table_setting())
            ctx.set_keyframe(G.device_setting(ofk, G.SET_STREAM))
            if seen:
                ctx.set_keyframe_rotation(device_rot(ofk, ROT_STREAM))
            ctx.stream_begin(frames[:, 0], cfg.to_params())
            for t in range(1, G.NF):
                if seen and t == 4:
                    assert (ctx.keyframe_rotation_download(G.B)[:, 3] == RR.OK).any()        # it was on, and solved
                    ctx.set_keyframe_rotation(None)
                out = ctx.stream_step(frames[:, t], sensors, cfg.to_params(), G.MC, G.RADIUS)
                d = ctx.keyframe_download(G.B, G.MC)
                if t >= 4:
                    rec = d["rec"].copy(); rec[:, 13:19] = 0.0
                    res.append(out + (dict(key_xy=d["key_xy"], member=d["member"], R_acc=d["R_acc"], rec=rec),))
        finally:
            ctx.close()
        return res
    a, b = run(True), run(False)
    assert np.array_equal(a[0][3]["rec"][:, 8], b[0][3]["rec"][:, 8])          # the same keyframes at the switch
    G.same(a, b, "off after on")


# ------------------------------------------------------------------------------------------------ (e) refusals
def test_rot_refusals_download_and_roundtrip(pkg, ofk):
    frames, info = G.frames_of(pkg)
    cfg, sensors = G.stream_cfg(), G.sensor_rows(ofk, info)
    ctx = ofk.Context(0, G.W, G.H, G.B, G.MC, cfg.max_level)
    try:
        r = ofk.keyframe_rotation_setting(source="attitude", axes=(1, 0, 1), sigma_gyro=1e-5, sigma_bias=2e-4, sigma_att=3e-3, iters=3, delta_max=0.05)
        ctx.set_keyframe_rotation(r)
        g = ctx.get_keyframe_rotation()
        assert (g.mode, g.source, list(g.axes), g.sigma_gyro, g.sigma_bias, g.sigma_att, g.iters, g.delta_max) == (1, 1, [1, 0, 1], 1e-5, 2e-4, 3e-3, 3, 0.05)
        with pytest.raises(ofk.OfkError):                          # nothing has stepped with the setting on
            ctx.keyframe_rotation_download(G.B)
        ctx.set_track_table(ofk.track_table_setting())
        ctx.stream_begin(frames[:, 0], cfg.to_params())
        with pytest.raises(ofk.OfkError) as e:                     # the keyframe is off: refused before any launch
            ctx.stream_step(frames[:, 1], sensors, cfg.to_params(), G.MC, G.RADIUS)
        assert e.value.code == ofk.E_INVALID and "ofk_set_keyframe" in str(e.value)
        with pytest.raises(ofk.OfkError):
            ctx.keyframe_rotation_download(G.B)
        ctx.set_keyframe(ofk.keyframe_setting())
        ctx.stream_step(frames[:, 1], sensors, cfg.to_params(), G.MC, G.RADIUS)
        q = ctx.keyframe_rotation_download(G.B)
        assert np.array_equal(q[:, 3], [RR.NONE] * G.B)          # the first step keys: nothing to refine yet
        st = {k: np.stack([RR.empty(8)[k]] * 1) for k in ("key_xy", "member", "state", "istate", "rstate")}
        args = (np.zeros((1, 8, 2), np.float32), np.ones((1, 8), np.uint8), [8], sensors[:1], np.zeros((1, 3)), [1], [0], st)
        with pytest.raises(ofk.OfkError):                          # the stage entry with the rotation off, and with a bad field
            ctx.keyframe_rotation_step(*args, rotation=ofk.keyframe_rotation_setting(False))
        with pytest.raises(ofk.OfkError):
            ctx.keyframe_rotation_step(*args, rotation=ofk.KeyframeRotation(1, 0, (1, 1, 1), 0.0, 1e-4, 1e-3, 0, 0.1))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ (f) a sequence through FlowStream
def test_rot_finite_motion_sequence_with_a_gyro_error(pkg, ofk):
    """test_gpu_keyframe's 12 frames of 240 x 320 through FlowStream with the track table, the templates, finite motion and the keyframe
    on, a gyro error of 1e-3 rad per frame in the sensors' omega, sigma_bias = 1e-3.  The CPU chain of the same frames
    (keyframe_rot_reference.rendered) ends 1.52e-3 d from the truth with the rotation and 1.66e-2 without (measured; the device: 1.55e-3 and 1.66e-2); the device's position
    with the rotation must lie within twice the CPU chain's (that test's tolerance for its own figure) and below the device's
    keyframe alone."""
    from of_amd.pipeline import FlowStream, PipelineConfig
    nf, size = 12, dict(h=240, w=320, corners=150)
    gerr = np.array([1e-3, -1e-3, 1e-3])
    rot = RR.setting(sigma_bias=1e-3)
    cpu = RR.rendered(nf, gerr, rot, **size)
    seq = K.rendered_sequence(nf, **size)
    errs = {}
    for name, kw in (("alone", {}), ("rot", dict(keyframe_rotation=device_rot(ofk, rot)))):
        cfg = PipelineConfig(max_corners=150, quality=0.01, min_distance=10, block_size=3, win=15, max_level=3, max_count=30, eps=0.01, min_eig_thr=1e-4,
                             track_table=True, track_template=True, finite_motion=True, keyframe=True, **kw)
        fs = FlowStream(320, 240, batch=1, cfg=cfg, min_features=0, mask_radius=5)
        try:
            fs.begin(seq["bgr"][None, 0])
            for j in range(1, nf):
                sn = K.rendered_sensors(seq, j); sn[4:7] += gerr
                fs.step(seq["bgr"][None, j], sn[None])
            p = fs.position()
            errs[name] = float(np.linalg.norm(p["pos"][0] - seq["truth"][nf - 1]) / seq["info"]["d"])
            if name == "rot":
                kq = fs.key_rotation()
                print("delta", kq["delta"], "flag", kq["flag"], "prior", kq["prior"], "iterations", kq["iterations"])
                assert kq["flag"][0] == ofk.KEYROT_OK and kq["iterations"][0] == 2 and p["flag"][0] == ofk.KEY_SOLVED
        finally:
            fs.close()
    print("position error / d at step", nf - 1, ": device", errs, "CPU chain", cpu)
    assert errs["rot"] <= 2.0 * cpu["rot"], (errs, cpu)
    assert errs["rot"] < errs["alone"], errs
