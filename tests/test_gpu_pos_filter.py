"""The position filter on the device (include/ofk.h: ofk_set_pos_filter) against its numpy restatement (tests/pos_filter_reference.py).
(a) the stage entry over the case table of tests/pos_filter_cases.py at batches of 1, 63, 64, 65 and 130 streams; (b) streams over
rendered sequences through ofk_stream_step and ofk_stream_step_fused; (c) the setting on against off; (d) refusals, reset and download,
the facades and optical_fusion.last_position.
Counts, outcome codes and flags are compared bit for bit; x, P and the record's f64 groups within REC_TOL of each group's scale, the
largest deviation met is printed as DEV.  Every step is compared on its own: the restatement starts from the state the device left."""
import dataclasses

import numpy as np
import pytest

import pos_filter_cases as PC
import pos_filter_reference as R
import test_gpu_keyframe as G
from test_gpu_keyframe import bits

pytestmark = pytest.mark.gpu
REC_TOL = 1e-9                                                   # the bound of test_gpu_epi.py and test_gpu_keyframe.py
DEV = dict(x=0.0, P=0.0, rec=0.0)


def device_setting(ofk, s):
    return ofk.pos_filter_setting(True, **s)


def group_dev(got, want, key, tag):
    scale = max(float(np.abs(want).max()), 1e-300)
    assert np.isfinite(want).all() and np.isfinite(got).all(), (tag, key, got, want)
    err = float(np.abs(got - want).max() / scale)
    DEV[key] = max(DEV[key], err)
    assert err <= REC_TOL, (tag, key, err, got, want)


def same_step(got_state, got_rec, want_state, want_rec, tag):
    """One stream's state and record behind one step."""
    assert np.array_equal(got_state["istate"], want_state["istate"]), (tag, got_state["istate"], want_state["istate"])
    assert np.array_equal(bits(got_rec[R.EXACT]), bits(want_rec[R.EXACT])), (tag, got_rec[R.EXACT], want_rec[R.EXACT])
    group_dev(got_state["x"], want_state["x"], "x", tag)
    group_dev(got_state["P"], want_state["P"], "P", tag)
    for name, sl in R.GROUPS.items():
        group_dev(got_rec[sl], want_rec[sl], "rec", (tag, name))
    assert np.array_equal(bits(got_rec[0:12]), bits(got_state["x"]))                 # the record carries the state it left


@pytest.fixture(scope="module")
def ctx(ofk):
    c = ofk.Context(0, 64, 48, 4, 64, 2)
    yield c
    c.close()
    print("DEV", DEV)


def run_group(ctx, ofk, group, B, pos0=(0.0, 0.0, 0.0)):
    """The group's scripts as B streams (cycled) through the stage entry, step by step -> the outcomes seen."""
    scripts = [group["scripts"][i % len(group["scripts"])] for i in range(B)]
    f = device_setting(ofk, group["setting"])
    states = [R.new_state(pos0) for _ in range(B)]
    state = {k: np.stack([s[k] for s in states]) for k in ("x", "P", "istate")}
    seen = set()
    for t in range(len(scripts[0]["steps"])):
        st = [sc["steps"][t] for sc in scripts]
        inp = np.stack([s["inp"] for s in st])
        keep = inp.copy()
        with np.errstate(all="ignore"):
            new, rec = ctx.pos_filter_step(np.stack([s["v"] for s in st]), [s["solved"] for s in st], np.stack([s["key"] for s in st]),
                                           np.stack([s["rw"] for s in st]), state=state, input=inp, pos_filter=f)
        assert np.array_equal(bits(inp), bits(keep))             # the caller's input row is not consumed: the device's copy is
        for b in range(B):
            want = {k: state[k][b].copy() for k in state}
            with np.errstate(all="ignore"):
                wrec = R.step(want, group["setting"], st[b]["v"], st[b]["solved"], st[b]["key"], st[b]["rw"], st[b]["inp"])
            same_step({k: new[k][b] for k in new}, rec[b], want, wrec, (group["name"], scripts[b]["name"], B, b, t))
            seen |= {(k, int(rec[b, 25 + 5 * k])) for k in range(3)}
        state = new
    return seen


# ------------------------------------------------------------------------------------------------ (a) the stage entry
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_stage_entry_at_the_wave_and_workgroup_edges(ctx, ofk, B):
    """The 32 combinations and the 24 broken inputs, cycled over B streams: one wave per stream, so 63 / 64 / 65 are a grid's edges."""
    run_group(ctx, ofk, PC.groups()[0], B)


def test_stage_entry_over_the_whole_case_table(ctx, ofk):
    seen = set()
    for g in PC.groups():
        seen |= run_group(ctx, ofk, g, max(len(g["scripts"]), 3), pos0=(0.5, -1.0, 2.0) if g["name"].startswith("share") else (0.0, 0.0, 0.0))
    assert seen == {(k, o) for k in range(3) for o in (R.NOT, R.APPLIED, R.GATED, R.REFUSED)}, seen
    print("DEV", DEV)


def test_a_second_launch_gives_the_same_bits_and_the_state_is_only_its_own(ctx, ofk):
    g = PC.groups()[0]
    a, b = [], []
    for out in (a, b):
        state = None
        for t in range(2):
            st = [sc["steps"][t] for sc in g["scripts"]]
            state, rec = ctx.pos_filter_step(np.stack([s["v"] for s in st]), [s["solved"] for s in st], np.stack([s["key"] for s in st]),
                                             np.stack([s["rw"] for s in st]), state=state, input=np.stack([s["inp"] for s in st]),
                                             pos_filter=device_setting(ofk, g["setting"]))
            out.append((state["x"].copy(), state["P"].copy(), state["istate"].copy(), rec.copy()))
    for p, q in zip(a, b):
        assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(p, q))


# ------------------------------------------------------------------------------------------------ (b) streams
POSF_STREAM = R.setting(sigma_v=2e-3, floor=1e-4, q_v=2e-3, p0_p=0.01, p0_v=0.05, nis_max=0.0)


class Follower:
    """The streams' filter restated from what the calls hand back: the step's record, ofk_keyframe_download, the sensors (the IMU
    state under use_imu) and the input handed in; compared with ofk_pos_filter_download after every call."""

    def __init__(self, ctx, nb, setting=POSF_STREAM):
        self.ctx, self.nb, self.s = ctx, nb, setting
        self.state = [R.new_state() for _ in range(nb)]
        self.rec = [None] * nb
        self.pending = np.zeros((nb, R.INPUT))
        self.outcomes = []

    def input(self, rows):
        self.ctx.pos_filter_input(rows)
        self.pending = np.array(rows, np.float64)

    def held(self, tag):
        d = self.ctx.pos_filter_download(self.nb)
        for b in range(self.nb):
            assert np.array_equal(bits(d["x"][b]), bits(self.state[b]["x"])) and np.array_equal(bits(d["P"][b]), bits(self.state[b]["P"])), tag
            assert np.array_equal(d["istate"][b], self.state[b]["istate"]) and np.array_equal(bits(d["rec"][b]), bits(self.rec[b])), tag

    def step(self, rec, sensors, fused, tag, imu=None):
        key = self.ctx.keyframe_download(self.nb, G.MC)["rec"]
        d = self.ctx.pos_filter_download(self.nb)
        for b in range(self.nb):
            rw = (sensors[b, 7:16] if imu is None else imu[b, 6:15]).reshape(3, 3)
            solved = int(rec[b, 15] != 0 if fused else rec[b, 4] >= 3)
            want = self.state[b]
            wrec = R.step(want, self.s, rec[b, 8:11], solved, key[b], rw, self.pending[b])
            got = {k: d[k][b] for k in ("x", "P", "istate")}
            same_step(got, d["rec"][b], want, wrec, (tag, b))
            self.state[b] = {k: got[k].copy() for k in got}      # the next step starts from the device's bits
            self.rec[b] = d["rec"][b].copy()
            self.outcomes.append(tuple(int(wrec[25 + 5 * k]) for k in range(3)) + (int(wrec[40]),))
        self.pending = np.zeros((self.nb, R.INPUT))              # consumed exactly once
        return d


def input_rows(nb, t):
    rows = np.zeros((nb, R.INPUT))
    rows[:, 0:3] = [1e-4 * t, -2e-4, 5e-5]
    rows[:, 3] = 1.0
    rows[:, 4:7] = np.array([0.012, -0.008, 0.004]) * t + 0.002
    rows[:, 7:10] = [0.004, 0.005, 0.006]
    if nb > 1:
        rows[1, 3] = 0.0                                         # a stream without a fix beside one with
    return rows


def run_stream(pkg, ofk, kind, posf, on_from=1):
    """kind: "plain" (ofk_stream_step, append re-detection) | "jpeg" (step 3 as JPEG) | "robust" | "replace" | "hold" | "imu" | "both"
    (the depths and the templates on as well).  posf: the filter on beside the keyframe, from step on_from on.  -> everything the
    calls returned and every other state's download, but the filter's own."""
    from of_amd.pipeline import FusionConfig
    frames, info = G.frames_of(pkg)
    nb = 1 if kind == "hold" else G.B
    frames = frames[:nb]
    fused = kind not in ("plain", "jpeg")
    cfg = G.stream_cfg(**(dict(robust="tukey", robust_drop=True) if kind == "robust" else {}))
    sensors = G.sensor_rows(ofk, info, nb)
    fusion = FusionConfig(use_imu=kind == "imu", redetect_replace=kind == "replace", hold_on_skip=kind == "hold")
    mf = G.MC - 10 if kind == "replace" else G.MC if not fused else G.MF
    ctx = ofk.Context(0, G.W, G.H, nb, G.MC, cfg.max_level)
    out, held = [], 0
    try:
        if kind == "robust":
            ctx.set_robust(cfg.robust_setting())
        ctx.imu_reset(nb)
        ctx.set_track_table(ofk.track_table_setting())
        if kind == "both":
            ctx.set_track_depth(ofk.track_depth_setting()); ctx.set_track_template(ofk.track_template_setting())
        ctx.set_keyframe(G.device_setting(ofk, G.SET_STREAM))
        tracks, counts = ctx.stream_begin(frames[:, 0], (cfg if fused else dataclasses.replace(cfg, max_corners=G.MC_BEGIN)).to_params())
        fol = None
        for t in range(1, G.NF):
            if posf and t == on_from:
                ctx.set_pos_filter(device_setting(ofk, POSF_STREAM))
                fol = Follower(ctx, nb)
            if fol and t in ((3, 6) if kind == "hold" else (2, 5, 6)):      # in front of a held step too: the input must survive it
                fol.input(input_rows(nb, t))
            fs = fusion.to_struct()
            if kind == "hold" and t in (3, 4):
                fs.min_solve = 10 ** 6
            if kind == "jpeg" and t == 3:
                rec, tracks, counts = ctx.stream_step_jpeg(G.jpeg_of(frames[:, t]), sensors, cfg.to_params(), mf, G.RADIUS)
                fz = None
            elif not fused:
                rec, tracks, counts = ctx.stream_step(frames[:, t], sensors, cfg.to_params(), mf, G.RADIUS)
                fz = None
            else:
                rec, fz, tracks, counts = ctx.stream_step_fused(frames[:, t], sensors, cfg.to_params(), fs, mf, G.RADIUS)
            hold = kind == "hold" and rec[0, 15] == 0
            extra = (ctx.keyframe_download(nb, G.MC),)
            if kind == "both":
                extra += (ctx.track_depth_download(nb, G.MC), {k: v for k, v in ctx.track_template_download(nb, G.MC).items() if k != "tmpl"})
            out.append((rec.copy(), tracks.copy(), counts.copy(), ctx.track_table_download(nb, G.MC)) + (() if fz is None else (fz.copy(),)) + extra)
            if fol:
                if hold:
                    held += 1
                    if fol.rec[0] is not None:
                        fol.held((kind, t, "held"))              # a held step launches nothing: state, record and input stay
                else:
                    fol.step(rec, sensors, fused, (kind, t), imu=ctx.imu_state(nb)[0] if kind == "imu" else None)
        if fol:
            o = fol.outcomes
            print(kind, "outcomes (v, D, fix, cloned)", o)
            assert sum(x[0] == R.APPLIED for x in o) >= 3 and sum(x[1] == R.APPLIED for x in o) >= 2 and sum(x[3] for x in o) >= 1, (kind, o)
            assert sum(x[2] == R.APPLIED for x in o) == (2 if kind == "hold" else 3 if on_from == 1 else 2), (kind, o)    # every fix once
            assert kind != "hold" or held >= 2
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("kind", ["plain", "robust", "both"])
def test_stream_steps_equal_the_restatement_and_change_nothing_else(pkg, ofk, kind):
    on = run_stream(pkg, ofk, kind, True)
    off = run_stream(pkg, ofk, kind, False)
    G.same(on, off, (kind, "filter on against keyframe alone"))
    print("DEV", DEV)


def test_stream_step_jpeg(pkg, ofk):
    pytest.importorskip("PIL.Image")
    run_stream(pkg, ofk, "jpeg", True)


@pytest.mark.parametrize("kind", ["replace", "hold", "imu"])
def test_fused_stream_kinds(pkg, ofk, kind):
    run_stream(pkg, ofk, kind, True)


def test_switched_on_in_mid_stream_and_off_after_on(pkg, ofk):
    """On from step 4: the filter starts there (rule 1 at its first step).  And a context that had the setting on for steps 1-3 returns
    from then on what one that never saw it returns: nothing reads the filter."""
    mid = run_stream(pkg, ofk, "plain", True, on_from=4)
    never = run_stream(pkg, ofk, "plain", False)
    G.same(mid, never, "on in mid-stream")
    frames, info = G.frames_of(pkg)
    cfg, sensors = G.stream_cfg(), G.sensor_rows(ofk, info)

    def run(seen):
        c = ofk.Context(0, G.W, G.H, G.B, G.MC, cfg.max_level)
        res = []
        try:
            c.set_track_table(ofk.track_table_setting())
            c.set_keyframe(G.device_setting(ofk, G.SET_STREAM))
            if seen:
                c.set_pos_filter(device_setting(ofk, POSF_STREAM))
            c.stream_begin(frames[:, 0], cfg.to_params())
            for t in range(1, G.NF):
                if seen and t == 4:
                    assert (c.pos_filter_download(G.B)["istate"][:, 0] == 3).all()
                    c.set_pos_filter(None)
                res.append(c.stream_step(frames[:, t], sensors, cfg.to_params(), G.MC, G.RADIUS) + (c.keyframe_download(G.B, G.MC), c.track_table_download(G.B, G.MC)))
            if seen:                                             # the state stays where the last step with the setting on left it
                assert (c.pos_filter_download(G.B)["istate"][:, 0] == 3).all()
        finally:
            c.close()
        return res
    G.same(run(True), run(False), "off after on")


# ------------------------------------------------------------------------------------------------ (d) refusals, reset, download, facades
def test_refusals_reset_and_download(pkg, ofk):
    frames, info = G.frames_of(pkg)
    cfg, sensors = G.stream_cfg(), G.sensor_rows(ofk, info)
    ctx = ofk.Context(0, G.W, G.H, G.B, G.MC, cfg.max_level)
    try:
        ctx.set_track_table(ofk.track_table_setting())
        ctx.set_pos_filter(device_setting(ofk, POSF_STREAM))
        ctx.stream_begin(frames[:, 0], cfg.to_params())
        with pytest.raises(ofk.OfkError) as e:                     # the keyframe is off: refused before any launch
            ctx.stream_step(frames[:, 1], sensors, cfg.to_params(), G.MC, G.RADIUS)
        assert e.value.code == ofk.E_INVALID and "ofk_set_keyframe" in str(e.value) and "ofk_set_pos_filter" in str(e.value)
        with pytest.raises(ofk.OfkError):                          # nothing was launched: no state yet
            ctx.pos_filter_download(G.B)
        ctx.set_keyframe(G.device_setting(ofk, G.SET_STREAM))
        with pytest.raises(ofk.OfkError):
            ctx.pos_filter_reset(G.B, None)
        with pytest.raises(ofk.OfkError):
            ctx.pos_filter_reset(0, [0.0, np.inf, 0.0])
        ctx.pos_filter_input(input_rows(G.B, 1))
        ctx.pos_filter_reset(1, [5.0, 6.0, 7.0])                 # before any step: the state begins, stream 1 at the given position
        d = ctx.pos_filter_download(G.B)
        assert np.array_equal(d["x"][:, 0:3], [[0, 0, 0], [5, 6, 7]]) and np.array_equal(d["x"][:, 9:12], d["x"][:, 0:3]) and not d["P"].any()
        assert np.array_equal(d["rec"][:, 0:12], d["x"]) and np.array_equal(d["istate"][:, 0:4], [[0, 1, 0, 0]] * 2)
        fol = Follower(ctx, G.B)
        fol.state[1] = R.new_state((5.0, 6.0, 7.0))
        fol.pending = input_rows(G.B, 1); fol.pending[1] = 0.0   # the reset cleared stream 1's input row, stream 0's waits
        rec, tracks, counts = ctx.stream_step(frames[:, 1], sensors, cfg.to_params(), G.MC, G.RADIUS)
        d = fol.step(rec, sensors, False, "after reset")
        assert np.array_equal(d["rec"][:, 47], [1, 1]) and np.array_equal(d["rec"][:, 35], [R.APPLIED, R.NOT]) and abs(d["x"][1, 0] - 5.0) < 0.1
        rec, tracks, counts = ctx.stream_step(frames[:, 2], sensors, cfg.to_params(), G.MC, G.RADIUS)
        d = fol.step(rec, sensors, False, "second step")
        assert np.array_equal(d["rec"][:, 47], [0, 0]) and np.array_equal(d["istate"][:, 0], [2, 2])
        ctx.pos_filter_reset(0, None)                            # in mid-stream: stream 0 starts over at zero, stream 1 goes on
        fol.state[0] = R.new_state()
        d2 = ctx.pos_filter_download(G.B)
        assert not d2["x"][0].any() and not d2["P"][0].any() and np.array_equal(bits(d2["x"][1]), bits(d["x"][1]))
        rec, tracks, counts = ctx.stream_step(frames[:, 3], sensors, cfg.to_params(), G.MC, G.RADIUS)
        d = fol.step(rec, sensors, False, "third step")
        assert np.array_equal(d["rec"][:, 47], [1, 0]) and np.array_equal(d["istate"][:, 0], [1, 3])
        ctx.stream_begin(frames[:, 0], cfg.to_params())          # ofk_stream_begin resets it
        with pytest.raises(ofk.OfkError):
            ctx.pos_filter_download(G.B)
        fol = Follower(ctx, G.B)
        rec, tracks, counts = ctx.stream_step(frames[:, 1], sensors, cfg.to_params(), G.MC, G.RADIUS)
        d = fol.step(rec, sensors, False, "after a new begin")
        assert np.array_equal(d["rec"][:, 47], [1, 1])
        st = R.new_state()
        args = (np.zeros((1, 3)), [1], R.key_record()[None], np.eye(3)[None])
        with pytest.raises(ofk.OfkError):                          # the stage entry with the setting off, and with a bad field
            ctx.pos_filter_step(*args, pos_filter=ofk.pos_filter_setting(False))
        with pytest.raises(ofk.OfkError):
            ctx.pos_filter_step(*args, pos_filter=ofk.PosFilter(1, 1.0, 1e-3, 0.0, 1.0, 1.5, 0.0, 1e-3, 0.0, 0.0, 1.0, 0.0, 0.0))
    finally:
        ctx.close()


def test_facades_return_the_context_step(pkg, ofk):
    import of_amd.simulation as sim
    import of_amd.velocity_node as node
    rng = np.random.default_rng(5)
    kw = dict(sigma_v=2e-3, share=0.25, p0_p=0.02)
    c = ofk.default_context()
    sn = sc = None
    full = None
    for t in range(3):
        s = PC.plain_step(rng, fix=t == 1, clone=t == 1)
        fix = dict(du=s["inp"][0:3]) if t != 1 else dict(du=s["inp"][0:3], fix=s["inp"][4:7], fix_sigma=s["inp"][7:10])
        sn, rn = node.pos_filter_step(s["v"], s["key"], s["rw"], state=sn, **fix, **kw)
        sc, rs = sim.pos_filter_step(s["v"], s["key"], s["rw"], state=sc, **fix, **kw)
        full, rec = c.pos_filter_step(s["v"][None], [1], s["key"][None], s["rw"][None], state=full, input=s["inp"][None], **kw)
        for got_state, got_rec in ((sn, rn), (sc, rs)):
            assert all(np.array_equal(bits(got_state[k]), bits(full[k][0])) for k in full) and np.array_equal(bits(got_rec), bits(rec[0]))
        assert rec[0, 42] == t + 1 and rec[0, 35] == (R.APPLIED if t == 1 else R.NOT)


def test_optical_fusion_fills_last_position(pkg, ofk):
    from of_amd import velocity_node as node
    frames, info = G.frames_of(pkg)
    m = node.optical_fusion(spin=False, synthetic_test=False, pos_filter=dict(sigma_v=2e-3, q_v=2e-3, q_p=0.05, p0_v=0.05))
    m.feature_params = dict(qualityLevel=0.01, minDistance=4, blockSize=5)
    m.T = 2.0
    assert m.last_position is None
    steps, applied = 0, []
    for t in range(G.NF):                                        # the node holds a step that did not solve: the filter then does not run,
        if t == 2:                                               # and the fix waits on the device for the next step that does
            m.call_fix([0.1, 0.2, 0.3], 0.01)
        m.call_optical(frames[0, t])
        if t:
            m.step()                                             # the main loop's pass: the next frame is taken only behind it
            fp = m._stream.fused_position()
            lp = m.last_position
            assert lp is not None and all(np.array_equal(bits(np.asarray(lp[k])), bits(np.asarray(fp[k][0]))) for k in ("p", "v", "c", "P", "rec", "outcome"))
            assert lp["counts"]["steps"] in (steps, steps + 1), (t, lp["counts"])
            if lp["counts"]["steps"] == steps + 1:
                steps += 1
                applied.append((t, int(lp["outcome"][2])))
                if lp["outcome"][2] == R.APPLIED:
                    assert np.abs(lp["p"] - [0.1, 0.2, 0.3]).max() < 0.02, lp["p"]       # the fix of sigma 0.01 pulled the position over
        assert m._fix is None
    first = [k for k, (t, o) in enumerate(applied) if t >= 2][0]
    assert steps >= 3 and [o for t, o in applied] == [R.NOT] * first + [R.APPLIED] + [R.NOT] * (len(applied) - first - 1), applied
    assert node.optical_fusion(spin=False, synthetic_test=False).last_position is None
