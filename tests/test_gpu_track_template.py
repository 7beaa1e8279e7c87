"""GPU: the track templates (include/ofk.h: ofk_set_track_template) against their restatement (tests/track_template_reference.py).

(1) ofk_track_template_step, rules 2-6, bit for bit (next, status, A and ncc as uint32, flag, tstate, the template bytes, the counts):
    windows 5 / 15 / 21 / 31; ten streams of 0, 1, 3, 4, 5, 63, 64, 65, 256, 257 rows in one launch (four rows per workgroup); positions
    on every fraction, and in a stream of their own 64 tracked rows on all 32 exact phases and all 32 exact ties in x and in y, scored at
    anchor_iters 0 and 3; windows whose footprint is one pixel inside and one pixel
    outside each border; A = identity, a rotation by 0.6 rad, scale 0.6 and 1.6, a shear, a NaN entry; a NaN position; templates of a
    constant region, a saturated region and a pure vertical edge; anchor_iters 0 and 8, outside keep and drop, rows with status 0,
    refresh at scale_max 1.2, appended rows through new_counts and max_total.
(2) ofk_track_affine_fit, rule 1, within 1e-10 relative: counts 0, 5, 6, 255, 256, 257, 1030, collinear points,
    30 % and 3 % of the rows displaced by 20 px, a NaN point, all status 0.
(3) stream chains equal the composition of stage entries on a second context: the frames from the resident pyramids, ofk_lk_pyr_fb /
    ofk_lk_pyr_light, the device's own L, ofk_track_template_step - ofk_stream_step with re-detection, step_fused with the robust
    drop and with zones, the replace re-detection, held steps, a JPEG step, the setting switched on in mid-stream, beside track_depth,
    lk_light, a camera and a seeded forward-backward gate.
(4) on against off: with ncc_min = -1, anchor_iters = 0 and outside = keep everything else a stream returns is the same bits; off
    after on equals a context that never saw the setting.
(5) the yaw sequence of the CPU experiment through FlowStream: the CPU reference's assertions hold for the device's tracks."""
import dataclasses
import io as _io
import zlib

import numpy as np
import pytest

import track_template_reference as T

pytestmark = pytest.mark.gpu
F = np.float32
KEYS = ("tmpl", "A", "ncc", "flag", "tstate")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def device_setting(ofk, s):
    return ofk.track_template_setting(True, s.win, s.ncc_min, s.anchor_iters, s.anchor_max, s.outside, s.fit_min, s.fit_gate, s.scale_max)


def same_state(got, want, count, win, tag):
    """The first `count` rows of two states: everything bit for bit; the template bytes of the rows that have one."""
    e2 = (win + 2) ** 2
    for k in ("A", "ncc", "flag", "tstate"):
        g, w = bits(got[k][:count]), bits(want[k][:count])
        assert np.array_equal(g, w), (tag, k, np.flatnonzero((g != w).reshape(count, -1).any(1))[:6])
    has = np.flatnonzero(want["tstate"][:count] != 0)
    assert np.array_equal(got["tmpl"][has, :e2], want["tmpl"][has, :e2]), (tag, "tmpl", has[(got["tmpl"][has, :e2] != want["tmpl"][has, :e2]).any(1)][:6])


# ------------------------------------------------------------------------------------------------ (1) the stage entry at its edges
H1, W1, S1 = 120, 160, 257
COUNTS1 = (0, 1, 3, 4, 5, 63, 64, 65, 256, 257)
MAPS = {"identity": (1, 0, 0, 1), "rotation": (np.cos(0.6), -np.sin(0.6), np.sin(0.6), np.cos(0.6)), "small": (0.6, 0, 0, 0.6), "large": (1.6, 0, 0, 1.6),
        "shear": (1, 0.3, 0, 1), "nan": (1, np.nan, 0, 1)}


@pytest.fixture(scope="module")
def ctx1(ofk):
    c = ofk.Context(0, W1, H1, len(COUNTS1), S1, 2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def images(pkg):
    """Two frames cut from one texture two pixels apart, with a constant, a saturated and a vertical-edge region in both."""
    from of_amd import synth
    tex = synth.make_texture(H1 + 8, W1 + 8, 21)
    tex = np.clip(np.rint(tex), 0, 255).astype(np.uint8)
    g0, g1 = tex[4:4 + H1, 4:4 + W1].copy(), tex[3:3 + H1, 2:2 + W1].copy()       # content moves by (+2, +1)
    for g, (dx, dy) in ((g0, (0, 0)), (g1, (2, 1))):
        g[8 + dy:48 + dy, 8 + dx:48 + dx] = 90                                     # constant
        g[8 + dy:48 + dy, 60 + dx:100 + dx] = 255                                  # saturated
        g[70 + dy:112 + dy, 8 + dx:29 + dx] = 40; g[70 + dy:112 + dy, 29 + dx:50 + dx] = 200      # a vertical edge at x = 29
    return g0, g1


def case_rows(rng, n, win, g0):
    """n rows of every kind the rules tell apart -> prev, next, status, age, state."""
    h = (win - 1) // 2
    lo, hix, hiy = h + 3.0, W1 - h - 6.0, H1 - h - 6.0
    prev = np.column_stack([rng.uniform(lo, hix, S1), rng.uniform(lo, hiy, S1)]).astype(F)
    nxt = (prev + F(2) * np.array([1, 0.5], F) + rng.uniform(-0.8, 0.8, (S1, 2)).astype(F)).astype(F)
    st = (rng.uniform(size=S1) < 0.9).astype(np.uint8) * rng.integers(1, 256, S1).astype(np.uint8)
    age = rng.integers(0, 5, S1).astype(np.int32)
    state = T.empty_state(S1, win)
    state["ncc"][:] = rng.uniform(-1, 1, S1); state["flag"][:] = rng.integers(0, 7, S1)
    names = list(MAPS)
    for r in range(S1):
        kind = r % 16
        ix, iy = np.floor(nxt[r])
        if kind == 0:                                            # some exact phases and ties among the other kinds (all of them: the test below)
            nxt[r] = (ix + (r // 16 % 32) / 32.0, iy + ((r // 16 * 7) % 32 + 0.5) / 32.0)
        elif kind == 1:
            nxt[r] = (ix + ((r // 16) % 32 + 0.5) / 32.0, iy + (r // 16 * 5 % 32) / 32.0)
        elif kind == 2:                                          # the footprint one pixel inside / outside each border
            edge = (r // 16) % 8
            inside = edge % 2 == 0
            x = {0: h + (0 if inside else -1), 1: W1 - 2 - h + (0 if inside else 1)}.get(edge // 2)
            y = {2: h + (0 if inside else -1), 3: H1 - 2 - h + (0 if inside else 1)}.get(edge // 2)
            nxt[r] = (nxt[r, 0] if x is None else x, nxt[r, 1] if y is None else y)
        elif kind == 3:                                          # the capture's footprint (one pixel wider) at the borders
            edge = (r // 16) % 8
            inside = edge % 2 == 0
            x = {0: h + 1 + (0 if inside else -1), 1: W1 - 3 - h + (0 if inside else 1)}.get(edge // 2)
            y = {2: h + 1 + (0 if inside else -1), 3: H1 - 3 - h + (0 if inside else 1)}.get(edge // 2)
            prev[r] = (prev[r, 0] if x is None else x, prev[r, 1] if y is None else y)
            age[r] = 0
        elif kind == 4:
            nxt[r, r // 16 % 2] = np.nan
        elif kind == 5:
            prev[r, 0] = np.nan; age[r] = 0
        # templates of the rows that have one: captured where the row was a few frames ago, or from the special regions
        if age[r] > 0 and rng.uniform() < 0.85:
            src = {6: (28, 28), 7: (80, 28), 8: (29, 90)}.get(kind)      # constant, saturated, the vertical edge
            if src is not None and win <= 31 and h + 1 <= 19:
                t = T.capture(g0, src[0], src[1], win)
                nxt[r] = (src[0] + 2 + rng.uniform(-0.4, 0.4), src[1] + 1 + rng.uniform(-0.4, 0.4))
            else:
                t = T.capture(g0, prev[r, 0] + rng.uniform(-0.3, 0.3), prev[r, 1] + rng.uniform(-0.3, 0.3), win)
            if t is not None:
                state["tmpl"][r, :len(t)] = t; state["tstate"][r] = 1
                m = np.array(MAPS[names[(r // 16) % len(names)] if kind in (9, 10, 11) else "identity"], np.float64)
                state["A"][r] = (m * (1 + rng.normal(0, 0.003, 4)) if kind >= 12 else m).astype(F)
        else:
            state["A"][r] = rng.normal(0, 1, 4)                  # noise: a row without a template reads none of it
    return prev, nxt, st, age, state


SETTINGS1 = {
    "win5": T.setting(win=5), "win15": T.setting(), "win21": T.setting(win=21), "win31": T.setting(win=31),
    "score-only-drop": T.setting(anchor_iters=0, outside=T.DROP, ncc_min=0.9), "eight-steps": T.setting(anchor_iters=8, anchor_max=1.0),
    "refresh-appended": T.setting(scale_max=1.2, outside=T.DROP),
}


@pytest.mark.parametrize("name", list(SETTINGS1))
def test_template_step_against_the_restatement(ctx1, ofk, images, name):
    s = SETTINGS1[name]
    g0, g1 = images
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    B = len(COUNTS1)
    rows = [case_rows(rng, n, s.win, g0) for n in COUNTS1]
    Ls = [np.array(m, F) for m in ((1, 0, 0, 1), (1.01, -0.02, 0.02, 0.99), (0.995, 0.01, -0.015, 1.002))]
    L = np.stack([Ls[b % 3] for b in range(B)])
    L[2] = (1, 0, np.nan, 1)                                     # a stream whose step map is no number: every sample is outside
    appended = name == "refresh-appended"
    new_counts = [(3 * b) % 11 for b in range(B)] if appended else None
    max_total = 250 if appended else None
    state = {k: np.stack([r[4][k] for r in rows]) for k in KEYS}
    nxt, st, got, rec = ctx1.track_template_step(np.stack([g0] * B), np.stack([g1] * B), np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]),
                                                 np.stack([r[2] for r in rows]), np.stack([r[3] for r in rows]), list(COUNTS1), L, state,
                                                 new_counts=new_counts, max_total=max_total, track_template=device_setting(ofk, s))
    seen = np.zeros(17, int)
    for b, (n, (prev, nx0, st0, age, state0)) in enumerate(zip(COUNTS1, rows)):
        wn, ws, wstate, wrec = T.template_step(g0, g1, prev, nx0, st0, age, n, L[b], state0, s, None if new_counts is None else new_counts[b], max_total)
        tag = (name, b, n)
        assert np.array_equal(bits(nxt[b]), bits(wn)), (tag, "next", np.flatnonzero((bits(nxt[b]) != bits(wn)).any(1))[:6])
        assert np.array_equal(st[b], ws), (tag, "status", np.flatnonzero(st[b] != ws)[:6])
        kept = int(np.count_nonzero(ws[:n]))
        count = kept + (0 if new_counts is None else max(0, min(new_counts[b], max_total - kept, S1 - kept)))
        same_state({k: got[k][b] for k in KEYS}, wstate, count, s.win, tag)
        assert np.array_equal(rec[b], wrec), (tag, rec[b, 10:20], wrec[10:20])
        seen[:10] += wrec[10:20].astype(int) > 0
    print(name, "streams in which each count of the record was met (scored .. largest move):", seen[:10])
    if name == "win15":
        assert (seen[:9] > 0).sum() >= 8, seen                   # every path but the refresh is met under the defaults
    if appended:
        assert seen[8] > 0                                       # rows marked for refresh


@pytest.mark.parametrize("iters", [0, 3])
def test_template_step_at_every_phase_and_every_tie(ctx1, ofk, images, iters):
    """All 32 exact fractional phases k / 32 and all 32 exact ties (k + 1/2) / 32, in x and in y: 64 tracked rows with a template and the
    identity map in a stream whose step map is the identity, so that the first sampling of every row sits exactly on its phase."""
    g0, g1 = images
    s = T.setting(anchor_iters=iters, ncc_min=-1.0)
    n = 64
    k = np.arange(n)
    fx, fy = k / 64.0, ((23 * k + 5) % 64) / 64.0                # every multiple of 1 / 64 once on each axis: even = a phase, odd = a tie
    assert sorted(fx * 64) == list(range(64)) and sorted(fy * 64) == list(range(64))
    base = np.column_stack([60 + 10 * (k % 8), 55 + 6 * (k // 8)]).astype(np.float64)     # textured ground, 16 px clear of every border
    nxt = (base + np.column_stack([fx, fy])).astype(F)
    assert np.array_equal(nxt.astype(np.float64), base + np.column_stack([fx, fy]))       # exact in f32
    prev = (nxt - np.array([2, 1], F)).astype(F)                 # where the content was in the previous frame
    state = T.empty_state(n, s.win)
    for r in range(n):
        t = T.capture(g0, prev[r, 0], prev[r, 1], s.win)
        state["tmpl"][r, :len(t)] = t; state["tstate"][r] = 1; state["A"][r] = (1, 0, 0, 1)
    st, age, L = np.ones(n, np.uint8), np.ones(n, np.int32), np.array([1, 0, 0, 1], F)
    gn, gs, got, rec = ctx1.track_template_step(g0[None], g1[None], prev[None], nxt[None], st[None], age[None], [n], L[None],
                                                {key: state[key][None] for key in KEYS}, track_template=device_setting(ofk, s))
    wn, ws, wstate, wrec = T.template_step(g0, g1, prev, nxt, st, age, n, L, state, s)
    assert wrec[10] == n and wrec[16] == 0 and (wstate["flag"][:n] == T.PASS).all() and wstate["ncc"][:n].min() > 0.9     # every row was scored, none captured
    ox, oy = T.offsets(s.win, (s.win - 1) // 2)
    for r in (1, 3):                                             # a tie rounds to even: 0.5 -> 0, 1.5 -> 2 in x
        sx = F(ox[0]) + nxt[r, 0]
        assert np.rint((sx - np.floor(sx)) * F(32)) == (0, 2)[r // 2] and (sx - np.floor(sx)) * F(32) == (0.5, 1.5)[r // 2]
    assert np.array_equal(bits(gn[0]), bits(wn)) and np.array_equal(gs[0], ws), np.flatnonzero((bits(gn[0]) != bits(wn)).any(1))
    same_state({key: got[key][0] for key in KEYS}, wstate, n, s.win, ("phases", iters))
    assert np.array_equal(rec[0], wrec), (rec[0, 10:20], wrec[10:20])
    if iters == 0:
        assert np.array_equal(bits(gn[0]), bits(nxt))            # scored where it stood


def test_python_stage_entry(pkg, ofk, images):
    """velocity_node.track_template_step: two frames through the facade, the state carried from call to call."""
    from of_amd import velocity_node
    g0, g1 = images
    rng = np.random.default_rng(11)
    prev = np.column_stack([rng.uniform(60, 150, 40), rng.uniform(52, 110, 40)]).astype(F)
    nxt = (prev + np.array([2, 1], F) + rng.uniform(-0.5, 0.5, (40, 2)).astype(F)).astype(F)
    p1, s1, state, rec = velocity_node.track_template_step(g0, g1, prev, nxt, new_count=3)
    cfg = T.setting()
    wrec, L = T.affine_fit(prev, nxt, np.ones(40, np.uint8), 40, H1, W1, cfg)
    pad = lambda a, *tail: np.concatenate([a, np.zeros((3,) + tail, a.dtype)])
    wn, ws, wstate, wrec2 = T.template_step(g0, g1, pad(prev, 2), pad(nxt, 2), pad(np.ones(40, np.uint8)), np.zeros(43, np.int32), 40,
                                            np.asarray(rec[0:4], F), T.empty_state(43, 15), cfg, 3, 43)
    kept = int(np.count_nonzero(ws[:40]))
    assert np.array_equal(bits(p1), bits(wn[:40])) and np.array_equal(s1, ws[:40]) and len(state["tstate"]) == kept + 3
    same_state(state, wstate, kept + 3, 15, "facade")
    assert np.allclose(rec[0:10], wrec[0:10], rtol=1e-10, atol=1e-10) and np.array_equal(rec[10:], wrec2[10:]) and rec[16] == 40
    assert np.abs(p1[s1 != 0] - (prev[s1 != 0] + np.array([2, 1], F))).max() < 0.1       # pulled back onto the content's true shift


# ------------------------------------------------------------------------------------------------ (2) the step map
S2 = 1030


@pytest.fixture(scope="module")
def ctx2(ofk):
    c = ofk.Context(0, W1, H1, 12, S2, 2)
    yield c
    c.close()


def affine_case(rng, n, kind="plain"):
    prev = (rng.random((S2, 2)) * (W1, H1)).astype(F)
    c = np.array([W1 / 2, H1 / 2])
    M = np.array([[1.01 * np.cos(0.02), -1.01 * np.sin(0.02)], [1.01 * np.sin(0.02), 1.01 * np.cos(0.02)]])
    nxt = ((prev - c) @ M.T + (1.5, -0.7) + c + rng.normal(0, 0.1, (S2, 2))).astype(F)
    st = (rng.uniform(size=S2) < 0.9).astype(np.uint8) * rng.integers(1, 256, S2).astype(np.uint8)
    if n <= 6:
        st[:] = 1                                                # 5 rows: one fewer than fit_min; 6: just enough
    if kind == "collinear":
        prev[:, 1] = 2 * prev[:, 0]; nxt = prev.copy()
    elif kind in ("many-off", "few-off"):
        k = rng.permutation(n)[:int(n * (0.3 if kind == "many-off" else 0.03))]
        nxt[k] += 20
    elif kind == "nan":
        st[7] = 1; nxt[7, 1] = np.nan
    elif kind == "untracked":
        st[:] = 0
    return prev, nxt, st, n


def test_affine_fit_against_the_restatement(ctx2, ofk):
    rng = np.random.default_rng(8)
    cases = [affine_case(rng, n) for n in (0, 5, 6, 255, 256, 257, 1030)]
    cases += [affine_case(rng, 400, k) for k in ("collinear", "many-off", "few-off", "nan", "untracked")]
    s = T.setting()
    rec, L = ctx2.track_affine_fit(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases]),
                                   [c[3] for c in cases], H1, W1, device_setting(ofk, s))
    worst = 0.0
    for b, (prev, nxt, st, n) in enumerate(cases):
        want, wL = T.affine_fit(prev, nxt, st, n, H1, W1, s)
        assert np.array_equal(rec[b, [6, 7, 8]], want[[6, 7, 8]]) and not rec[b, 10:].any(), (b, rec[b], want)
        scale = np.maximum(1.0, np.abs(want[:10]))
        err = float((np.abs(rec[b, :10] - want[:10]) / scale).max())
        worst = max(worst, err)
        assert err <= 1e-10, (b, rec[b, :10], want[:10])
        assert np.array_equal(bits(L[b]), bits(rec[b, 0:4].astype(F)))               # L is M rounded once
    print("step map: largest relative deviation from the restatement", worst)
    flags = rec[:, 6]
    assert list(flags[:3]) == [1, 1, 0] and flags[7] == 1 and flags[10] == 1 and flags[11] == 1      # too few rows, collinear, NaN, none tracked
    assert rec[8, 8] < 0.7 * rec[8, 7] and 0.9 * rec[9, 7] < rec[9, 8] < rec[9, 7]                  # what the gate does with 30 % and with 3 % off
    r1, _ = ctx2.track_affine_fit(cases[9][0][None], cases[9][1][None], cases[9][2][None], [400], H1, W1, device_setting(ofk, T.setting(fit_gate=0.0)))
    w1, _ = T.affine_fit(cases[9][0], cases[9][1], cases[9][2], 400, H1, W1, T.setting(fit_gate=0.0))
    assert r1[0, 8] == 0 and np.allclose(r1[0, :10], w1[:10], rtol=1e-10, atol=1e-10)


# ------------------------------------------------------------------------------------------------ (3), (4) streams
H, W, NF, B = 120, 160, 8, 2
MOTION = dict(v=(0.012, -0.008, 0.004), omega=(0.002, -0.001, 0.03), d=1.0)
MC, MF, RADIUS, MC_BEGIN = 120, 100, 5, 100
LEVELS = 2
_frames = {}


def frames_of(pkg):
    if "f" not in _frames:
        from of_amd import synth
        seqs = [synth.render_sequence(H, W, 60 + b, NF, margin=64, **MOTION) for b in range(B)]
        _frames["f"] = (np.stack([s[0] for s in seqs]), seqs[0][1])
    return _frames["f"]


def stream_cfg(**kw):
    from of_amd.pipeline import PipelineConfig
    return PipelineConfig(max_corners=MC, quality=0.01, min_distance=4, block_size=5, win=15, max_level=LEVELS, max_count=20, eps=0.03, min_eig_thr=1e-4, **kw)


def sensor_rows(ofk, info, n=B):
    return ofk.make_sensors(n, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"], v_prior=info["v"])


class Follower:
    """The templates of a context's streams as the composition of stage entries on a second context (`stage`), advanced with what
    the stream calls hand back and compared with the device's after every call."""

    def __init__(self, ofk, ctx, stage, s, gate=None, light=None):
        self.ofk, self.ctx, self.stage, self.s, self.gate, self.light = ofk, ctx, stage, s, gate, light
        self.scored = self.moved = self.dropped = self.captured = 0

    def start(self, tracks, counts, age=None):
        self.B = len(counts)
        self.pos = [tracks[b, :counts[b]].copy() for b in range(self.B)]
        self.age = [np.zeros(counts[b], np.int32) if age is None else age[b][:counts[b]].copy() for b in range(self.B)]
        self.state = [T.empty_state(MC, self.s.win) for _ in range(self.B)]
        return self

    def replaced(self, b, n):
        self.age[b] = np.zeros(n, np.int32)

    def step(self, tracks, counts, tag, held=False):
        ofk, nb = self.ofk, self.B
        d = self.ctx.track_template_download(nb, MC)
        table = self.ctx.track_table_download(nb, MC)
        nxt_dev, keep = self.ctx.stream_last_points(MC)
        slot = (0, 1) if held else (1, 0)                        # a step that is not held swaps the frames behind it
        g0 = np.stack([self.ctx.resident_pyramid(slot[0], b, H, W, 0)[0] for b in range(nb)])
        g1 = np.stack([self.ctx.resident_pyramid(slot[1], b, H, W, 0)[0] for b in range(nb)])
        n_old = [len(p) for p in self.pos]
        pad = lambda rows, dtype, *tail: np.stack([np.concatenate([np.asarray(r, dtype), np.zeros((MC - len(r),) + tail, dtype)]) for r in rows])
        prev = pad(self.pos, F, 2)
        lk = self.stage.lk_pyr_fb(g0, g1, prev, n_old, gate=self.gate if self.gate is not None else ofk.track_gate_setting(), win=15, max_level=LEVELS,
                                  light=self.light)
        L = d["rec"][:, 0:4].astype(F)                           # the device's own step map ...
        for b in range(nb):                                      # ... which is the restatement's to rounding
            want, _ = T.affine_fit(prev[b], lk["next_pts"][b], lk["status"][b], n_old[b], H, W, self.s)
            err = float((np.abs(d["rec"][b, :10] - want[:10]) / np.maximum(1.0, np.abs(want[:10]))).max())
            assert np.array_equal(d["rec"][b, [6, 7]], want[[6, 7]]) and err <= 1e-10, (tag, b, d["rec"][b, :10], want[:10])
        state = {k: np.stack([st[k] for st in self.state]) for k in KEYS}
        age = pad(self.age, np.int32)
        setting = device_setting(ofk, self.s)
        new = [int(counts[b]) - int(np.count_nonzero(keep[b, :n_old[b]])) for b in range(nb)]
        nA, sA, stA, recA = self.stage.track_template_step(g0, g1, prev, lk["next_pts"], lk["status"], age, n_old, L, state, new_counts=new, max_total=MC,
                                                           track_template=setting)
        for b in range(nb):
            n = n_old[b]
            assert np.array_equal(bits(nxt_dev[b, :n]), bits(nA[b, :n])), (tag, b, "next")
            assert not np.any((keep[b, :n] != 0) & (sA[b, :n] == 0)), (tag, b, "a row the templates dropped is kept")
        if held:                                                 # rule 6 has not run: what had a template keeps everything
            for b in range(nb):
                had = np.flatnonzero(self.state[b]["tstate"][:n_old[b]] != 0)
                for k in KEYS:
                    assert np.array_equal(d[k][b][had], self.state[b][k][had]), (tag, b, k, "held")
                e2 = (self.s.win + 2) ** 2
                for r in np.flatnonzero((self.state[b]["tstate"][:n_old[b]] == 0) & (d["tstate"][b, :n_old[b]] != 0)):
                    # a row without a template that the held step captured: the bits the next step would have captured
                    assert np.array_equal(d["tmpl"][b, r, :e2], T.capture(g0[b], prev[b, r, 0], prev[b, r, 1], self.s.win)), (tag, b, r, "held capture")
                    assert np.array_equal(d["A"][b, r], np.array([1, 0, 0, 1], F)), (tag, b, r)
                    for k in ("tmpl", "A", "tstate"):
                        self.state[b][k][r] = d[k][b, r]
            return d
        solve_dropped = any(np.any((keep[b, :n_old[b]] != 0) != (sA[b, :n_old[b]] != 0)) for b in range(nb))
        flags = [10, 11, 12, 13, 14, 15, 16, 17, 19]             # from the flags and the moves alone, whatever the solve dropped behind them
        assert np.array_equal(d["rec"][:, flags], recA[:, flags]), (tag, d["rec"][:, 10:20], recA[:, 10:20])
        if solve_dropped:                                        # rule 6 ran on what the solve left: the same rows scored, fewer kept
            _, _, stA, recB = self.stage.track_template_step(g0, g1, prev, lk["next_pts"], ((keep != 0) & (lk["status"] != 0)).astype(np.uint8), age, n_old, L,
                                                          state, new_counts=new, max_total=MC, track_template=setting)
            assert np.array_equal(d["rec"][:, 18], recB[:, 18]), (tag, "refresh", d["rec"][:, 18], recB[:, 18])
        else:
            assert np.array_equal(d["rec"][:, 10:], recA[:, 10:]), (tag, d["rec"][:, 10:20], recA[:, 10:20])
        for b in range(nb):
            assert np.array_equal(table["age"][b, :counts[b]] > 0, np.arange(counts[b]) < counts[b] - new[b]), (tag, b, "ages")
            same_state({k: d[k][b] for k in KEYS}, {k: stA[k][b] for k in KEYS}, int(counts[b]), self.s.win, (tag, b))
            self.state[b] = {k: stA[k][b].copy() for k in KEYS}
            self.pos[b] = tracks[b, :counts[b]].copy()
            self.age[b] = table["age"][b, :counts[b]].copy()
        r = d["rec"]
        self.scored += int(r[:, 10].sum()); self.dropped += int(r[:, 11].sum()); self.moved += int(r[:, 12].sum()); self.captured += int(r[:, 16].sum())
        return d


def jpeg_of(batch):
    from PIL import Image
    res = []
    for img in batch:
        buf = _io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=92)
        res.append(buf.getvalue())
    return res


NEUTRAL = T.setting(ncc_min=-1.0, anchor_iters=0, outside=T.KEEP)


def run_plain(pkg, ofk, s, jpeg_step=None, on_from=1, off_from=None):
    """ofk_stream_step over the steps; the streams begin with MC_BEGIN corners and re-detect up to MC whenever they hold fewer; s: the
    setting (None: never on), on from step on_from, off again from off_from.  -> everything the calls returned."""
    frames, info = frames_of(pkg)
    cfg, sensors = stream_cfg(), sensor_rows(ofk, info)
    ctx, stage = ofk.Context(0, W, H, B, MC, LEVELS), ofk.Context(0, W, H, B, MC, LEVELS)
    out, fol = [], None
    try:
        ctx.set_track_table(ofk.track_table_setting())
        tracks, counts = ctx.stream_begin(frames[:, 0], dataclasses.replace(cfg, max_corners=MC_BEGIN).to_params())
        out.append((tracks.copy(), counts.copy()))
        for t in range(1, NF):
            if s is not None and t == on_from:
                ctx.set_track_template(device_setting(ofk, s))
                fol = Follower(ofk, ctx, stage, s).start(tracks, counts, None if t == 1 else ctx.track_table_download(B, MC)["age"])
            if t == off_from:
                ctx.set_track_template(None)
                fol = None
            if t == jpeg_step:
                rec, tracks, counts = ctx.stream_step_jpeg(jpeg_of(frames[:, t]), sensors, cfg.to_params(), MC, RADIUS)
            else:
                rec, tracks, counts = ctx.stream_step(frames[:, t], sensors, cfg.to_params(), MC, RADIUS)
            out.append((rec.copy(), tracks.copy(), counts.copy(), ctx.track_table_download(B, MC)))
            if fol:
                fol.step(tracks, counts, ("plain", t))
        if fol and s is not NEUTRAL:
            print("plain: rows scored", fol.scored, "moved", fol.moved, "dropped", fol.dropped, "captured", fol.captured)
            assert fol.scored > 100 and fol.moved > 50 and fol.captured >= int(out[0][1].sum())
    finally:
        ctx.close(); stage.close()
    return out


def same(a, b, tag):
    assert len(a) == len(b), tag
    for k, (x, y) in enumerate(zip(a, b)):
        for i, (p, q) in enumerate(zip(x, y)):
            if isinstance(p, dict):
                assert all(np.array_equal(p[key], q[key]) for key in p), (tag, k, i)
            else:
                assert np.array_equal(p.view(np.uint8), q.view(np.uint8)), (tag, k, i)


def test_stream_step_is_the_composition(pkg, ofk):
    run_plain(pkg, ofk, T.setting())


def test_neutral_setting_is_off_for_everything_else(pkg, ofk):
    off = run_plain(pkg, ofk, None)
    same(run_plain(pkg, ofk, NEUTRAL), off, "plain: neutral against off")
    same(run_plain(pkg, ofk, NEUTRAL, off_from=4), off, "plain: off after on against never on")


def test_stream_step_jpeg(pkg, ofk):
    pytest.importorskip("PIL.Image")
    run_plain(pkg, ofk, T.setting(), jpeg_step=3)


def test_setting_switched_on_in_the_middle_of_a_stream(pkg, ofk):
    run_plain(pkg, ofk, T.setting(), on_from=4)


def run_fused(pkg, ofk, s, kind):
    """ofk_stream_step_fused on the sensors, no filter.  kind: "robust" (the robust solve drops its outliers from the tracks) |
    "zones" | "replace" (streams with few tracks replace them in front of LK) | "hold" (one stream; steps 3 and 4 are not solved and
    held) | "depth" | "light" | "camera" | "gate" (a seeded forward-backward gate)."""
    from of_amd.pipeline import CameraModel, FusionConfig
    frames, info = frames_of(pkg)
    nb = 1 if kind == "hold" else B
    frames = frames[:nb]
    robust = kind in ("robust", "zones")
    cfg = stream_cfg(**(dict(robust="tukey", robust_drop=True) if robust else {}))
    sensors = sensor_rows(ofk, info, nb)
    fusion = FusionConfig(redetect_replace=kind == "replace", hold_on_skip=kind == "hold")
    cam = CameraModel(fx=160.0, fy=160.0, cx=80.0, cy=60.0, k=(-0.1, 0.01, 0, 0)) if kind == "camera" else None
    if cam is not None:
        sensors[:, 19:22] = cam.sensor_slots()
    gate = ofk.track_gate_setting(fb="seeded", fb_thr=1.0) if kind == "gate" else None
    light = "gain" if kind == "light" else None
    mf = MC if kind == "replace" else MF                      # replace: every stream that has room replaces its tracks, at every step
    ctx, stage = ofk.Context(0, W, H, nb, MC, LEVELS), ofk.Context(0, W, H, nb, MC, LEVELS)
    out, events = [], 0
    try:
        if robust:
            ctx.set_robust(cfg.robust_setting())
        if kind == "zones":
            ctx.set_zones(ofk.zones_setting(link=24, min_members=2, radius=8, ttl=4))
        if cam is not None:
            ctx.set_camera(cam.setting())
        if gate is not None:
            ctx.set_track_gate(gate)
        if light is not None:
            ctx.set_lk_light(light)
        ctx.imu_reset(nb)
        ctx.set_track_table(ofk.track_table_setting())
        if kind == "depth":
            ctx.set_track_depth(ofk.track_depth_setting())
        if s is not None:
            ctx.set_track_template(device_setting(ofk, s))
        tracks, counts = ctx.stream_begin(frames[:, 0], cfg.to_params())
        fol = Follower(ofk, ctx, stage, s, gate=gate, light=light).start(tracks, counts) if s is not None else None
        for t in range(1, NF):
            fs = fusion.to_struct()
            if kind == "hold" and t in (3, 4):
                fs.min_solve = 10 ** 6                           # more points than there are: not solved
            before = counts.copy()
            rec, fused, tracks, counts = ctx.stream_step_fused(frames[:, t], sensors, cfg.to_params(), fs, mf, RADIUS)
            hold = kind == "hold" and rec[0, 15] == 0
            out.append((rec.copy(), fused.copy(), tracks.copy(), counts.copy(), ctx.track_table_download(nb, MC)) +
                       ((ctx.zones_download(nb),) if kind == "zones" else ()) + ((ctx.track_depth_download(nb, MC),) if kind == "depth" else ()))
            if fol:
                if kind == "replace":                            # the streams that replaced their tracks did so in front of LK: their rows are the new corners
                    table = ctx.track_table_download(nb, MC)
                    for b in range(nb):
                        if before[b] <= mf and MC - before[b] > 0:
                            step_pts = _replaced_points(ctx, b, MC - int(before[b]), cfg)
                            assert len(step_pts) == table["stats"][b, 1] + table["stats"][b, 2]     # kept + lost = the rows this step tracked
                            fol.pos[b], fol.age[b] = step_pts, np.zeros(len(step_pts), np.int32)
                            events += 1
                fol.step(tracks, counts, (kind, t), held=hold)
                events += int(hold)
        if fol:
            print(kind, "rows scored", fol.scored, "moved", fol.moved, "dropped", fol.dropped, "captured", fol.captured, "events", events)
            if s is not NEUTRAL:
                assert fol.scored > 50 and fol.moved > 20
            if kind in ("replace", "hold"):
                assert events >= (2 if kind == "hold" else 1), (kind, events)
    finally:
        ctx.close(); stage.close()
    return out


def _replaced_points(ctx, b, budget, cfg):
    """The corners a replace re-detection put in front of LK: k_redetect_limits' budget, detected on the previous frame (behind the
    step: pyramid slot 1) by the reference loop's detection."""
    from oracle import image_oracle as io
    g_prev = ctx.resident_pyramid(1, b, H, W, 0)[0]
    return io.good_features(g_prev, budget, cfg.quality, cfg.min_distance, cfg.block_size).reshape(-1, 2).astype(F)


@pytest.mark.parametrize("kind", ["robust", "zones"])
def test_stream_step_fused_with_robust_drop(pkg, ofk, kind):
    run_fused(pkg, ofk, T.setting(), kind)
    same(run_fused(pkg, ofk, NEUTRAL, kind), run_fused(pkg, ofk, None, kind), (kind, "neutral against off"))


def test_stream_replace_redetection(pkg, ofk):
    run_fused(pkg, ofk, T.setting(), "replace")


def test_held_steps_leave_the_templates(pkg, ofk):
    run_fused(pkg, ofk, T.setting(), "hold")


@pytest.mark.parametrize("kind", ["depth", "light", "camera", "gate"])
def test_composition(pkg, ofk, kind):
    run_fused(pkg, ofk, T.setting(), kind)
    if kind == "depth":
        same(run_fused(pkg, ofk, NEUTRAL, kind), run_fused(pkg, ofk, None, kind), (kind, "neutral against off"))


def test_refusal_without_the_table(pkg, ofk):
    frames, info = frames_of(pkg)
    cfg, sensors = stream_cfg(), sensor_rows(ofk, info)
    ctx = ofk.Context(0, W, H, B, MC, LEVELS)
    try:
        ctx.stream_begin(frames[:, 0], cfg.to_params())
        ctx.set_track_template(ofk.track_template_setting())
        for call in (lambda: ctx.stream_step(frames[:, 1], sensors, cfg.to_params(), MC, RADIUS),):
            with pytest.raises(ofk.OfkError) as e:
                call()
            assert e.value.code == ofk.E_INVALID
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ (5) the yaw sequence on the device
def test_yaw_sequence_through_flowstream(pkg, ofk):
    from of_amd.pipeline import FlowStream, PipelineConfig
    seq = T.sequence("yaw")
    info = seq["info"]
    sensors = ofk.make_sensors(1, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"], v_prior=info["v"])
    res = {}
    for kind, tpl in (("lk", None), ("score", ofk.track_template_setting(anchor_iters=0)), ("on", True)):
        cfg = PipelineConfig(max_corners=T.CORNERS, quality=0.01, min_distance=10, block_size=3, win=15, max_level=3, track_table=True, track_template=tpl)
        fs = FlowStream(T.W_SEQ, T.H_SEQ, batch=1, cfg=cfg, min_features=0, mask_radius=5)
        try:
            tracks, counts = fs.begin(seq["bgr"][None, 0])
            birth = {int(i): tracks[0, r].astype(np.float64) for r, i in enumerate(fs.track_table()["ids"][0])}
            for k in range(1, len(seq["bgr"])):
                _, tracks, counts = fs.step(seq["bgr"][None, k], sensors)
            ids = fs.track_table()["ids"][0]
            Hk = np.linalg.matrix_power(seq["H"], len(seq["bgr"]) - 1)
            truth = T.project(Hk, np.array([birth[int(i)] for i in ids]))
            res[kind] = T.summary(dict(err=np.hypot(*(tracks[0, :counts[0]].astype(np.float64) - truth).T)))
            if tpl is True:
                t = fs.templates()
                assert len(t["ids"][0]) == counts[0] and t["tmpl"][0].shape == (counts[0], 17, 17)
        finally:
            fs.close()
    on, lk, score = res["on"], res["lk"], res["score"]
    print(f"yaw on the device, step 29: LK alone {lk}, LK + score {score}, templates on {on}")
    assert on[0] <= 0.1 and on[0] <= 0.2 * lk[0] and on[0] <= 0.2 * score[0]
    assert on[2] > lk[2] and on[3] >= score[3]
