"""GPU: the track table (include/ofk.h: ofk_set_track_table) against its restatement (tests/track_table_reference.py), bit for bit.

(a) ofk_track_table_step at the update kernel's edges: counts around the 64-lane and 256-row boundaries, status patterns that keep
    all, none, a random set, only the last or only the first row of every chunk, appended rows none / some / more than the budget
    (kept == max_total included), three streams of different counts in one call.
(b) ofk_track_seed_points: ages 0 and >= 1 mixed, gain 1 and 0.5, a seed beyond 1e6 and a NaN flow falling back to the point, age-0
    rows keeping a model seed.
(c) streams on the frames of tests/point_count_cases.py: step (landing on 256 and 257 tracks), step_fused with the robust drop,
    without and with the exclusion zones on, the replace re-detection, hold_on_skip with unsolved steps, a JPEG step - after every
    call the downloaded table equals the restatement fed with the call's previous tracks, ofk_stream_last_points' next points and
    keep flags and the returned tracks.
    A stream that meets the setting in the middle of its life starts its table there.
(d) off is off: the same runs with the table on (seed off), with the setting off, and on a context that had it on and then off
    return the same tracks, counts, records, fused rows and zone tables.
(e) seed "flow" is a composition: the step's next points and keep flags equal ofk_lk_pyr_fb / ofk_lk_pyr_light started at positions
    built on the host from the table downloaded before the step - alone, beside lk_seed "model", beside a camera model, beside a
    "seeded" forward-backward gate, under lk_light "gain".  (A stream hands out no err, so err is not compared.)
(f) the ramp experiment's translation row through a one-stream context: the CPU reference's per-step good counts, and its conditions."""
import dataclasses
import io as _io
import zlib

import numpy as np
import pytest

import point_count_cases as P
import track_table_reference as T
from point_count_cases import bits
from oracle import image_oracle as io

pytestmark = pytest.mark.gpu
KEYS = ("ids", "age", "birth_step", "birth_xy", "flow_xy")


@pytest.fixture(scope="module")
def ctx(ofk):
    c = ofk.Context(0, 64, 48, 3, 1100, 2)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ (a) the update kernel's edges
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1030)
PATTERNS = ("all", "none", "random", "chunk-last", "chunk-first")
S_EDGE = 1030


def status_of(pattern, n, rng):
    i = np.arange(S_EDGE)
    st = {"all": np.ones(S_EDGE, bool), "none": np.zeros(S_EDGE, bool), "random": rng.uniform(size=S_EDGE) < 0.6,
          "chunk-last": (i % 256 == 255) | (i == n - 1), "chunk-first": i % 256 == 0}[pattern]
    return (st * rng.integers(1, 256, S_EDGE)).astype(np.uint8)  # any non-zero byte keeps; rows beyond n are noise


def random_table(rng, n):
    """A table in the middle of its life: `n` rows with shuffled ids, and stale rows behind them."""
    t = T.empty(S_EDGE)
    t["ids"][:] = rng.permutation(5000)[:S_EDGE] + 7
    t["age"][:] = rng.integers(0, 40, S_EDGE); t["birth_step"][:] = rng.integers(0, 90, S_EDGE)
    t["birth_xy"][:] = rng.uniform(0, 600, (S_EDGE, 2)); t["flow_xy"][:] = rng.normal(0, 20, (S_EDGE, 2))
    t["step"], t["next_id"], t["count"] = 90, 6000, n
    return t


def run_step(ctx, ofk, tabs, prev, nxt, st, new, new_counts, max_total, setting):
    B = len(tabs)
    table = {k: np.stack([t[k] for t in tabs]) for k in KEYS}
    head = np.array([[t["step"], t["next_id"]] for t in tabs], np.int32)
    counts = [t["count"] for t in tabs]
    return ctx.track_table_step(table, head, prev, nxt, st, counts, None if new_counts is None else new, new_counts, max_total, setting)


def check_step(ctx, ofk, ns, pattern, appended, seed, case):
    rng = np.random.default_rng(zlib.crc32(repr((tuple(ns), pattern, appended)).encode()))
    B = len(ns)
    tabs = [random_table(rng, n) for n in ns]
    prev = rng.uniform(0, 600, (B, S_EDGE, 2)).astype(np.float32); nxt = (prev + rng.normal(0, 15, prev.shape)).astype(np.float32)
    st = np.stack([status_of(pattern, n, rng) for n in ns])
    new = rng.uniform(0, 600, (B, S_EDGE, 2)).astype(np.float32)
    kept = [int(np.count_nonzero(st[b, :ns[b]])) for b in range(B)]
    if appended == "none":
        new_counts, max_total = None, S_EDGE
    elif appended == "some":
        new_counts, max_total = [17 + b for b in range(B)], S_EDGE
    elif appended == "clamped":                                  # more than max_total - kept: the budget cuts them
        max_total = min(S_EDGE, max(kept) + 5)
        new_counts = [40] * B
    else:                                                        # "full": kept == max_total in stream 0 (more in none): nothing fits
        max_total = kept[0]
        new_counts = [9] * B
    setting = ofk.TrackTable(1, 1, 0.5) if seed else None
    got, head, counts, sid, stats = run_step(ctx, ofk, tabs, prev, nxt, st, new, new_counts, max_total, setting)
    for b in range(B):
        want, wsid, wstats = T.update(tabs[b], prev[b], nxt[b], st[b], new[b], None if new_counts is None else new_counts[b], max_total,
                                      seed=seed, gain=0.5)
        tag = (case, "stream", b, "n", ns[b], "kept", kept[b], "max_total", max_total)
        assert np.array_equal(stats[b], wstats), (tag, stats[b], wstats)
        assert counts[b] == want["count"] and list(head[b]) == [want["step"], want["next_id"]], tag
        for k in KEYS:                                           # the whole stride: rows behind the count keep what they held
            assert np.array_equal(bits(got[k][b]), bits(want[k])), (tag, k, P.differing(got[k][b], want[k])[:4])
        assert np.array_equal(sid[b, :ns[b]], wsid) and not sid[b, ns[b]:].any(), tag
        if appended == "clamped":
            assert stats[b][3] == min(40, max_total - kept[b]) and (kept[b] < max(kept) or stats[b][3] == max_total - kept[b] < 40), tag
        if appended == "full" and b == 0:
            assert stats[b][3] == 0 and stats[b][0] == kept[b], tag


@pytest.mark.parametrize("pattern", PATTERNS)
def test_update_kernel_edges(ctx, ofk, pattern):
    """Every count under one status pattern, the four kinds of appends in turn, three streams per call."""
    kinds = ("none", "some", "clamped", "full")
    groups = [COUNTS[i:i + 3] for i in range(0, len(COUNTS), 3)]
    for g, ns in enumerate(groups):
        for a, appended in enumerate(kinds):
            check_step(ctx, ofk, ns, pattern, appended, seed=(g + a) % 2 == 1, case=(pattern, appended))


def test_update_three_streams_of_different_counts(ctx, ofk):
    for ns in ((1030, 0, 257), (1, 513, 64), (300, 300, 299)):
        check_step(ctx, ofk, ns, "random", "clamped", True, ("mixed", ns))


# ------------------------------------------------------------------------------------------------ (b) the seed kernel's edges
@pytest.mark.parametrize("gain", [1.0, 0.5])
def test_seed_kernel_edges(ctx, ofk, gain):
    rng = np.random.default_rng(3)
    S, ns = 600, (600, 257, 0)
    pts = rng.uniform(0, 640, (3, S, 2)).astype(np.float32)
    age = rng.integers(0, 3, (3, S)).astype(np.int32)
    flow = rng.normal(0, 30, (3, S, 2)).astype(np.float32)
    age[0, :8] = (1, 1, 5, 1, 0, 0, 1, 2)
    flow[0, 0] = (3e6, 1); flow[0, 1] = (1, -3e6); flow[0, 2] = (np.nan, 2); flow[0, 3] = (2, np.inf); flow[0, 4] = (np.nan, np.nan)
    pts[0, 6] = (999999.5, 10); flow[0, 6] = (0.5 / gain, 0)      # lands on 1e6 exactly: inside
    pts[0, 7] = (999999.5, 10); flow[0, 7] = (1.0 / gain, 0)      # one f32 step beyond: the point
    model = (pts + rng.normal(0, 5, pts.shape)).astype(np.float32)
    for given in (None, model):
        got = ctx.track_seed_points(pts, ns, age, flow, gain, seed=given)
        for b in range(3):
            want = T.seed_points(pts[b], ns[b], age[b], flow[b], gain, None if given is None else given[b])
            assert np.array_equal(bits(got[b]), bits(want)), (gain, given is None, b, P.differing(got[b], want)[:4])
    w0 = T.seed_points(pts[0], 600, age[0], flow[0], gain, model[0])
    assert all(np.array_equal(w0[i], pts[0, i]) for i in (0, 1, 2, 3, 7)) and np.array_equal(w0[6], np.float32([1e6, 10]))
    assert np.array_equal(w0[4], model[0, 4]) and np.array_equal(w0[5], model[0, 5])                 # age 0: the model seed stays
    old = age[0] >= 1
    assert np.count_nonzero(old) > 100 and np.count_nonzero(~old) > 100 and not np.array_equal(w0[old][10:], pts[0][old][10:])


# ------------------------------------------------------------------------------------------------ (c), (d) streams
class Follower:
    """The restated tables of a context's streams, advanced with what the calls hand back and compared after every call."""

    def __init__(self, ctx, tracks, counts, S, seed=False, gain=1.0, resident=True):
        self.ctx, self.B, self.S, self.seed, self.gain = ctx, len(counts), S, seed, gain
        self.t, self.stats, self.pos = [], [], []
        for b in range(self.B):
            t, st = T.begin(tracks[b, :counts[b]], int(counts[b]), S)
            self.t.append(t); self.stats.append(st); self.pos.append(tracks[b, :counts[b]].copy())
        if resident:                                             # else: the device starts its table with the next step
            self.compare("begin")

    def compare(self, tag, step_ids=None):
        d = self.ctx.track_table_download(self.B, self.S)
        for b in range(self.B):
            n = self.t[b]["count"]
            assert np.array_equal(d["stats"][b], self.stats[b]), (tag, b, d["stats"][b], self.stats[b])
            for k in KEYS:
                assert np.array_equal(bits(d[k][b, :n]), bits(self.t[b][k][:n])), (tag, b, k, P.differing(d[k][b, :n], self.t[b][k][:n])[:4])
            if step_ids is not None:
                assert np.array_equal(d["step_ids"][b, :len(step_ids[b])], step_ids[b]), (tag, b, "step_ids")
        return d

    def replaced(self, b, new_pts):
        self.t[b], self.stats[b] = T.replace(self.t[b], new_pts, len(new_pts))
        self.pos[b] = np.asarray(new_pts, np.float32).reshape(-1, 2).copy()

    def step(self, tracks, counts, max_total, tag, held=False):
        if held:                                                 # rule 4 (a replace in front of it has happened)
            self.compare((tag, "held"))
            return
        nxt, keep = self.ctx.stream_last_points(self.S)
        sids = []
        for b in range(self.B):
            n_old = self.t[b]["count"]
            assert n_old == len(self.pos[b]), (tag, b)
            kp = keep[b, :n_old] != 0
            kept = int(kp.sum())
            assert np.array_equal(bits(tracks[b, :kept]), bits(nxt[b, :n_old][kp])), (tag, b, "the kept tracks are the next points")
            app = tracks[b, kept:counts[b]]
            self.t[b], sid, self.stats[b] = T.update(self.t[b], self.pos[b], nxt[b, :n_old], keep[b, :n_old], app, len(app), max_total,
                                                     seed=self.seed, gain=self.gain)
            assert self.t[b]["count"] == counts[b], (tag, b)
            self.pos[b] = tracks[b, :counts[b]].copy()
            sids.append(sid)
        self.compare(tag, sids)


def apply_mode(ctx, ofk, mode):
    """mode: "on" (the table, seed off) | "off" | "on-off" (a context that had the setting on, then off)."""
    if mode in ("on", "on-off"):
        ctx.set_track_table(ofk.track_table_setting())
    if mode == "on-off":
        ctx.set_track_table(None)


def run_plain(ofk, mode, jpeg=None):
    """ofk_stream_step over the (300, 256) run of point_count_cases: stream 0 lands on 256, then on 257 tracks.  -> everything the
    calls returned."""
    run = P.stream_run("edges", 300, 256)
    frames, _ = P.stream_frames(False)
    cfg, sensors, B = run["cfg"], run["sensors"], P.B_STREAMS
    S = max(mc for mc, _ in run["asked"])
    ctx = ofk.Context(0, P.W, P.H, B, S, cfg.max_level)
    out = []
    try:
        apply_mode(ctx, ofk, mode)
        enc = jpeg or (lambda f: f)
        tracks, counts = (ctx.stream_begin_jpeg(enc(frames[:, 0]), cfg.to_params()) if jpeg else ctx.stream_begin(frames[:, 0], cfg.to_params()))
        out.append((tracks.copy(), counts.copy()))
        fol = Follower(ctx, tracks, counts, S) if mode == "on" else None
        crossed = set()
        for t, (mc, mf) in enumerate(run["asked"] if not jpeg else run["asked"][:2], start=1):
            params = dataclasses.replace(cfg, max_corners=mc).to_params()
            if jpeg:
                rec, tracks, counts = ctx.stream_step_jpeg(enc(frames[:, t]), sensors, params, mf, P.MASK_RADIUS)
            else:
                rec, tracks, counts = ctx.stream_step(frames[:, t], sensors, params, mf, P.MASK_RADIUS)
            out.append((rec.copy(), tracks.copy(), counts.copy()))
            if fol:
                fol.step(tracks, counts, mc, ("step", t))
                crossed |= {int(c) for c in counts}
        if fol and not jpeg:
            assert {256, 257} <= crossed and max(s[3] for s in fol.stats) > 0, crossed      # both sides of a chunk; rows were appended
            assert any(t["age"][:t["count"]].max() == len(run["asked"]) for t in fol.t)       # a track as old as the stream
    finally:
        ctx.close()
    return out


def same(a, b, tag):
    assert len(a) == len(b), tag
    for k, (x, y) in enumerate(zip(a, b)):
        for i, (u, v) in enumerate(zip(x, y)):
            if isinstance(u, dict):
                assert all(np.array_equal(u[key], v[key]) for key in u), (tag, k, i)
            else:
                assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), (tag, k, i)


def test_stream_step_across_256_and_off_is_off(pkg, ofk):
    on = run_plain(ofk, "on")
    same(on, run_plain(ofk, "off"), "on against off")
    same(on, run_plain(ofk, "on-off"), "on against on-then-off")


def test_stream_step_jpeg(pkg, ofk):
    Image = pytest.importorskip("PIL.Image")

    def enc(batch):
        res = []
        for img in batch:
            buf = _io.BytesIO()
            Image.fromarray(img).save(buf, "JPEG", quality=90)
            res.append(buf.getvalue())
        return res
    run_plain(ofk, "on", jpeg=enc)


def run_fused_robust(ofk, mode, zones):
    """ofk_stream_step_fused with the robust solve dropping its outliers from the tracks; zones: the exclusion zones grow from them."""
    from of_amd.pipeline import FusionConfig
    frames, info = P.stream_frames(False)
    cfg, B, mf = P.stream_cfg(600, "robust-fused", True), P.B_STREAMS, 590
    sensors, fusion = P.sensor_rows(info), FusionConfig(use_imu=False)
    ctx = ofk.Context(0, P.W, P.H, B, 600, cfg.max_level)
    out = []
    try:
        ctx.set_robust(cfg.robust_setting())
        if zones:
            ctx.set_zones(ofk.zones_setting(link=24, min_members=2, radius=8, ttl=4))
        ctx.imu_reset(B)
        apply_mode(ctx, ofk, mode)
        tracks, counts = ctx.stream_begin(frames[:, 0], cfg.to_params())
        fol = Follower(ctx, tracks, counts, 600) if mode == "on" else None
        dropped = 0
        for t in range(1, 5):
            rec, fused, tracks, counts = ctx.stream_step_fused(frames[:, t], sensors, cfg.to_params(), fusion.to_struct(), mf, P.MASK_RADIUS)
            out.append((rec.copy(), fused.copy(), tracks.copy(), counts.copy()) + ((ctx.zones_download(B),) if zones else ()))
            if fol:
                fol.step(tracks, counts, 600, ("fused", zones, t))
                dropped += int(sum(rec[b, 13] - s[1] for b, s in enumerate(fol.stats)))      # tracked by LK, not kept
        if fol:
            assert dropped > 0, "the robust drop took no track: the keep flags were LK's status"
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("zones", [False, True], ids=["plain", "zones"])
def test_stream_step_fused_with_robust_drop(pkg, ofk, zones):
    on = run_fused_robust(ofk, "on", zones)
    same(on, run_fused_robust(ofk, "off", zones), "fused: on against off")
    if zones:
        print("zones inserted per step:", [int(o[4]["stats"][:, 1].sum()) for o in on])


def test_stream_replace_redetection(pkg, ofk):
    """of_module's loop: streams with few tracks replace them in front of LK; the replaced rows get fresh ids."""
    from of_amd.pipeline import FusionConfig
    m = P.module_run("edges")
    frames, _ = P.stream_frames(False)
    cfg, B, mf = P.module_cfg(), P.B_STREAMS, P.MODULE_MIN_FEATURES
    fusion = FusionConfig.of_module(synthetic_flow=False)
    ctx = ofk.Context(0, P.W, P.H, B, cfg.max_corners, cfg.max_level)
    try:
        ctx.imu_reset(B); ctx.filter_configure(fusion.model, B)
        ctx.set_track_table(ofk.track_table_setting())
        tracks, counts = ctx.stream_begin(frames[:, 0], cfg.to_params())
        fol = Follower(ctx, tracks, counts, cfg.max_corners)
        replaced = 0
        for t in range(1, P.NF):
            sensors = np.concatenate([ofk.make_sensors(1, d=1.0, normal=m["normal"], omega=m["omegas"][t - 1, b], scaling=1.0, cx=m["cx"], cy=m["cy"])
                                      for b in range(B)])
            sensors[:, 25:28] = m["controls"][t - 1]
            for b in range(B):                                   # k_redetect_limits' rule, the detection of the reference loop
                budget = cfg.max_corners - fol.t[b]["count"]
                if fol.t[b]["count"] <= mf and budget > 0:
                    g_prev = io.gray_bgr8(frames[b, t - 1])
                    fol.replaced(b, io.good_features(g_prev, budget, cfg.quality, cfg.min_distance, cfg.block_size).reshape(-1, 2))
                    replaced += 1
            rec, fused, tracks, counts = ctx.stream_step_fused(frames[:, t], sensors, cfg.to_params(), fusion.to_struct(), mf, P.MASK_RADIUS)
            fol.step(tracks, counts, cfg.max_corners, ("replace", t))
            for b in range(B):
                assert rec[b, 12] == fol.stats[b][1] + fol.stats[b][2], ("replace", t, b)
        assert replaced >= 8 and all(t["next_id"] > 1000 for t in fol.t), replaced
    finally:
        ctx.close()


def test_held_steps_leave_the_table(pkg, ofk):
    """hold_on_skip: the clip of tests/test_gpu_fused.py whose threshold gives held and solved steps."""
    from of_amd import synth
    from of_amd.of_library import pix_trans
    from of_amd.pipeline import PipelineConfig, FusionConfig
    h, w, nf = 240, 320, 9
    frames, info = synth.render_sequence(h, w, 41, nf, v=(0.006, -0.004, 0.002), omega=(0.001, -0.002, 0.003), d=1.0)
    rng = np.random.default_rng(13)
    controls = rng.normal(0, 0.01, (nf - 1, 3)); omegas = rng.normal(0, 0.01, (nf - 1, 3))
    cx, cy = pix_trans((240, 320))
    cfg = PipelineConfig.of_module(); cfg.max_corners = 60; cfg.quality = 0.05; cfg.block_size = 7; cfg.min_distance = 8; cfg.max_level = 2; cfg.feas_T = 0.8
    fusion = FusionConfig.of_module(synthetic_flow=False, hold_on_skip=True)
    ctx = ofk.Context(0, w, h, 1, 60, 2)
    try:
        ctx.imu_reset(1); ctx.filter_configure(fusion.model, 1)
        ctx.set_track_table(ofk.track_table_setting())
        tracks, counts = ctx.stream_begin(frames[0][None], cfg.to_params())
        fol = Follower(ctx, tracks, counts, 60)
        held = solved = 0
        prev_frame = 0
        for t in range(1, nf):
            sensors = ofk.make_sensors(1, d=1.0, normal=(0, 0, 1), omega=omegas[t - 1], scaling=1.0, cx=cx, cy=cy)
            sensors[:, 25:28] = controls[t - 1]
            budget = 60 - fol.t[0]["count"]
            if fol.t[0]["count"] <= 10 and budget > 0:
                fol.replaced(0, io.good_features(io.gray_bgr8(frames[prev_frame]), budget, cfg.quality, cfg.min_distance, cfg.block_size).reshape(-1, 2))
            rec, fused, tracks, counts = ctx.stream_step_fused(frames[t][None], sensors, cfg.to_params(), fusion.to_struct(), 10, 10)
            hold = rec[0, 15] == 0
            held += hold; solved += not hold
            fol.step(tracks, counts, 60, ("hold", t), held=hold)
            if not hold:
                prev_frame = t
        assert held >= 1 and solved >= 2 and fol.t[0]["step"] == solved, (held, solved)
    finally:
        ctx.close()


def test_setting_switched_on_in_the_middle_of_a_stream(pkg, ofk):
    """Streams that step with the setting on without a table of their current tracks start one there by rule 1 - after a begin
    without the setting, and again after a step with the setting off - and ofk_stream_begin starts a new one."""
    frames, info = P.stream_frames(False)
    cfg, B, S = P.stream_cfg(300), P.B_STREAMS, 300
    sensors = P.sensor_rows(info)
    ctx = ofk.Context(0, P.W, P.H, B, S, cfg.max_level)
    try:
        tracks, counts = ctx.stream_begin(frames[:, 0], cfg.to_params())
        _, tracks, counts = ctx.stream_step(frames[:, 1], sensors, cfg.to_params(), 256, P.MASK_RADIUS)
        with pytest.raises(ofk.OfkError):
            ctx.track_table_download(B)
        for t in (2, 4):                                         # on for a step, off for a step, on again
            ctx.set_track_table(ofk.track_table_setting())
            fol = Follower(ctx, tracks, counts, S, resident=False)
            _, tracks, counts = ctx.stream_step(frames[:, t], sensors, cfg.to_params(), 256, P.MASK_RADIUS)
            fol.step(tracks, counts, 300, ("switched on", t))
            assert all(s[5] == 1 and s[4] <= 1 for s in fol.stats), t                # the table's first step: no track is older
            ctx.set_track_table(None)
            _, tracks, counts = ctx.stream_step(frames[:, t + 1], sensors, cfg.to_params(), 256, P.MASK_RADIUS)
        ctx.set_track_table(ofk.track_table_setting())
        tracks, counts = ctx.stream_begin(frames[:, 0], cfg.to_params())
        Follower(ctx, tracks, counts, S)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ (e) the seed is a composition
COMPOSE = ("alone", "lk-seed-model", "camera", "gate-seeded", "light-gain")


@pytest.mark.parametrize("beside", COMPOSE)
def test_flow_seed_is_a_composition(pkg, ofk, gpu_ctx, beside):
    from of_amd.pipeline import CameraModel
    frames, info = P.stream_frames(False)
    B, S, gain = 2, 300, 0.75
    cfg = P.stream_cfg(300)
    cfg.max_level = 1
    frames = frames[:B]
    cam = CameraModel(fx=320.0, fy=320.0, cx=160.0, cy=120.0, k=(-0.1, 0.01, 0, 0)).setting() if beside == "camera" else None
    model = beside in ("lk-seed-model", "camera")
    gate = ofk.track_gate_setting(fb="seeded", fb_thr=0.5, fb_level=0) if beside == "gate-seeded" else ofk.track_gate_setting()
    light = "gain" if beside == "light-gain" else None
    sensors = P.sensor_rows(info, B)
    if cam is not None:
        sensors[:, 19:22] = CameraModel(fx=320.0, fy=320.0, cx=160.0, cy=120.0, k=(-0.1, 0.01, 0, 0)).sensor_slots()
    ctx = ofk.Context(0, P.W, P.H, B, S, 3)
    try:
        ctx.set_track_table(ofk.track_table_setting("flow", gain))
        if model:
            ctx.set_lk_seed("model", 1.0)
        if cam is not None:
            ctx.set_camera(cam)
        if beside == "gate-seeded":
            ctx.set_track_gate(gate)
        if light:
            ctx.set_lk_light(light)
        tracks, counts = ctx.stream_begin(frames[:, 0], cfg.to_params())
        fol = Follower(ctx, tracks, counts, S, seed=True, gain=gain)
        moved = 0
        for t in range(1, 5):
            before = ctx.track_table_download(B, S)
            prev = np.zeros((B, S, 2), np.float32)
            prev[:, :tracks.shape[1]] = tracks
            n = counts.copy()
            start = None
            if model:                                            # what k_seed_points leaves in front of k_track_seed
                ideal = gpu_ctx.undistort_points(cam, prev, n) if cam is not None else prev
                start = gpu_ctx.predict_points(ideal, n, sensors, ofk.SEED_MODEL, 1.0)
                if cam is not None:
                    start = gpu_ctx.distort_points(cam, start, n)
            init = np.stack([T.seed_points(prev[b], int(n[b]), before["age"][b], before["flow_xy"][b], gain, None if start is None else start[b])
                             for b in range(B)])
            g0 = gpu_ctx.gray_bgr8(frames[:, t - 1]); g1 = gpu_ctx.gray_bgr8(frames[:, t])
            want = gpu_ctx.lk_pyr_fb(g0, g1, prev, n, gate, cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr, next_pts=init,
                                     flags=ofk.LK_USE_INITIAL_FLOW, light=light)
            rec, tracks, counts = ctx.stream_step(frames[:, t], sensors, cfg.to_params(), 0, P.MASK_RADIUS)
            nxt, keep = ctx.stream_last_points(S)
            for b in range(B):
                tag = (beside, "step", t, "stream", b)
                assert np.array_equal(bits(nxt[b, :n[b]]), bits(want["next_pts"][b, :n[b]])), (tag, P.differing(nxt[b, :n[b]], want["next_pts"][b, :n[b]])[:4])
                assert np.array_equal(keep[b, :n[b]], want["status"][b, :n[b]]), tag
                old = before["age"][b, :n[b]] >= 1
                moved += int(np.count_nonzero((init[b, :n[b]] != prev[b, :n[b]]).any(1) & old))
                if t == 1:
                    assert not old.any() and (model or np.array_equal(init[b], prev[b])), tag
            fol.step(tracks, counts, cfg.max_corners, (beside, t))
            if t > 1:
                assert all(s[7] > 0 for s in fol.stats), (beside, t, [s[7] for s in fol.stats])
        assert moved > 100, moved
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ (f) the experiment on the device
def test_ramp_experiment_on_the_device(pkg, ofk):
    """The translation row through ofk_stream_begin / ofk_stream_step with seed "flow": step 1 at maxLevel 3 (no track has a flow
    yet), then maxLevel 1.  LK parity is bit-exact, so the good counts are the CPU reference's."""
    from of_amd.pipeline import PipelineConfig
    name = "translation"
    seq = T.experiment_sequence(name)
    cpu = T.run_experiment(name, 1, True)
    cfg = PipelineConfig(max_corners=300, quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, **{k: v for k, v in T.EXP_LK.items() if k != "win"})
    bgr = [np.repeat(f[..., None], 3, 2) for f in seq["frames"]]
    sensors = ofk.make_sensors(1, scaling=1.0 / 640, cx=320, cy=240)
    ctx = ofk.Context(0, T.W_EXP, T.H_EXP, 1, 300, 3)
    try:
        ctx.set_track_table(ofk.track_table_setting("flow"))
        tracks, counts = ctx.stream_begin(bgr[0][None], cfg.to_params())
        assert counts[0] == len(seq["pts"]) and np.array_equal(tracks[0, :counts[0]], seq["pts"])
        got = []
        for k in range(len(T.RAMP)):
            n = int(counts[0])
            prev = tracks[0, :n].copy()
            params = dataclasses.replace(cfg, max_level=3 if k == 0 else 1).to_params()
            rec, tracks, counts = ctx.stream_step(bgr[k + 1][None], sensors, params, -1, 10)
            nxt, keep = ctx.stream_last_points(300)
            got.append(T.lsr.good_points(T.step_points(seq, k, prev), nxt[0, :n], keep[0, :n]))
        stats = ctx.track_table_download(1)["stats"][0]
    finally:
        ctx.close()
    print("device, seeded maxLevel 1:", " ".join("%d/%d" % r for r in got))
    assert got == cpu, (got, cpu)
    assert min(T.shares(got)) >= T.SEEDED_MIN_GOOD
    assert T.shares(T.run_experiment(name, 3, False))[-1] <= T.shares(got)[-1] - T.PLAIN_GAP
    assert stats[3] == 0 and stats[4] == len(T.RAMP) and stats[7] > 0             # no births; the survivors are 12 steps old
