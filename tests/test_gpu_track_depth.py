"""GPU: the depth per track (include/ofk.h: ofk_set_track_depth) against its restatement (tests/track_depth_reference.py).

(a) ofk_track_depth_step at the kernel's edges: counts around the 64-lane and 256-row boundaries at stride 1030, status patterns that
    keep all, none, a random set, only the first or only the last row of every chunk, appended rows none / some / past max_total /
    kept == max_total, three streams per launch with a v, an omega and a solved flag each.  rho, var, nobs and the counts agree bit for
    bit (the arithmetic is + - * / only); v_map and C_map within test_gpu_epi.py's REC_TOL of their slot group's scale (same sums, a
    Jacobi against numpy's eigh).  The largest deviation met is printed (-s) for the README.
(b) three streams of different counts in one launch.
(c) every skip and reset path of the stage entry, each one seen to count: |b| < b_min, the cross-flow gate, the innovation gate,
    z <= 0 on a row without a depth, g < 0.1, an unsolved record, update = 0, gate = 0, NaN and infinity in a point.
(d) streams over rendered 128 x 160 sequences, 8 steps: ofk_stream_step with re-detection, a JPEG step, the setting switched on in
    the middle of a stream; ofk_stream_step_fused with the robust drop, without and with the zones, with the replace re-detection,
    with held steps.  After every call the downloaded state equals the restatement fed with the points, keep flags, sensors and
    records the calls handed back.
(e) on against off: records, fused rows, tracks, counts and the track table are the same bits.
(f) composition: beside the epipolar solve, a camera model (the ideal points) and use_imu (the IMU state's omega).
(g) refusals: the track table off, OFK_SOLVE_OFMODULE, OFK_FLOW_ROTATIONAL, OFK_KEEP_LEGACY.
(h) a plane sequence through the device chain: after 8 steps the mature rows' depths lie within 3 sqrt(var) of the plane's inverse
    depth on the share of rows that the CPU run of the same frames through the C oracle chain reaches (measured first: 1.0 of 114
    and of 107 rows), the restatement equality after each step."""
import dataclasses
import io as _io
import zlib

import numpy as np
import pytest

import epi_reference as er
import track_depth_reference as T
from test_gpu_epi import REC_TOL
from oracle import image_oracle as io

pytestmark = pytest.mark.gpu
KEYS = ("rho", "var", "nobs")
DEV = [0.0]                                                      # the largest deviation of v_map / C_map met, in units of the slot group's scale


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_record(got, want, tag):
    exact = [3, 4, 5, 6, 7, 8, 9, 16, 17, 18, 19, 20] + list(range(21, T.TD_DOUBLES))
    assert np.array_equal(bits(got[exact]), bits(want[exact])), (tag, got, want)
    close = [0, 1, 2, 10, 11, 12, 13, 14, 15]                   # v_map and C_map
    err = (np.abs(got - want) / T.record_scale(want))[close]
    DEV[0] = max(DEV[0], float(err.max()))
    assert err.max() <= REC_TOL, (tag, close[int(err.argmax())], got[close], want[close])


@pytest.fixture(scope="module")
def ctx(ofk):
    c = ofk.Context(0, 64, 48, 3, 1100, 2)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ (a), (b) the kernel's edges
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 513, 1030)
PATTERNS = ("all", "none", "random", "chunk-first", "chunk-last")
S_EDGE = 1030
SET = T.setting(sigma_flow=er.SIGMA_FLOW, b_min=0.5e-3, q=1e-9)


def device_setting(ofk, s):
    return ofk.track_depth_setting(True, s["sigma_flow"], s["b_min"], s["gate"], s["q"], s["min_obs"], s["rel_max"], s["min_rows"], s["update"])


def status_of(pattern, n, rng):
    i = np.arange(S_EDGE)
    st = {"all": np.ones(S_EDGE, bool), "none": np.zeros(S_EDGE, bool), "random": rng.uniform(size=S_EDGE) < 0.6,
          "chunk-last": (i % 256 == 255) | (i == n - 1), "chunk-first": i % 256 == 0}[pattern]
    return (st * rng.integers(1, 256, S_EDGE)).astype(np.uint8)  # any non-zero byte keeps; rows beyond n are noise


def scene(rng, S=S_EDGE):
    """A stream in the middle of its life: points over the frame, the flow of (V, OM) over relief with noise and a few wild rows, a
    state whose rows have 0..11 measurements, most of them close to the truth, some far (the innovation gate), some not mature."""
    x = rng.uniform(-1.0, 1.0, (S, 2)) * [T.W2, T.H2]
    rho_true = rng.uniform(0.5, 1.4, S)
    u = er.flow(x, er.V, er.OM, rho_true) + rng.normal(0, er.SIGMA_FLOW, (S, 2))
    wild = rng.uniform(size=S) < 0.05
    u[wild] += rng.normal(0, 3e-3, (int(wild.sum()), 2))
    nobs = rng.integers(0, 12, S).astype(np.int32)
    rho = rho_true * (1.0 + rng.normal(0, 0.01, S)) * np.where(rng.uniform(size=S) < 0.03, 1.3, 1.0)
    var = (rng.uniform(0.002, 0.4, S) * rho) ** 2
    rho[nobs == 0] = 0.0; var[nobs == 0] = 0.0
    v = er.V * (1.0 + rng.normal(0, 0.003, 3)); om = er.OM + rng.normal(0, 1e-4, 3)
    return x, u, dict(rho=rho, var=var, nobs=nobs), v, om


def run_stage(ctx, ofk, cases, s, new_counts, max_total):
    """cases: per stream (x, u, status, n, omega, v, solved, state).  -> the device's (state, rec) and the restatement's per stream."""
    st = {k: np.stack([c[7][k] for c in cases]) for k in KEYS}
    got, rec = ctx.track_depth_step(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases]),
                                    [c[3] for c in cases], np.stack([c[4] for c in cases]), np.stack([c[5] for c in cases]),
                                    [int(c[6]) for c in cases], st, new_counts=new_counts, max_total=max_total, track_depth=device_setting(ofk, s))
    want = [T.step(c[7], c[0], c[1], c[2], c[3], c[4], c[5], c[6], s, None if new_counts is None else new_counts[b], max_total)
            for b, c in enumerate(cases)]
    return got, rec, want


def compare_stage(got, rec, want, tag):
    for b, (wst, wrec, count, _) in enumerate(want):
        for k in KEYS:
            assert np.array_equal(bits(got[k][b, :count]), bits(wst[k][:count])), (tag, b, k, np.flatnonzero(bits(got[k][b, :count]) != bits(wst[k][:count]))[:4])
        same_record(rec[b], wrec, (tag, b))


def check_step(ctx, ofk, ns, pattern, appended, case):
    rng = np.random.default_rng(zlib.crc32(repr((tuple(ns), pattern, appended)).encode()))
    cases = []
    for b, n in enumerate(ns):
        x, u, state, v, om = scene(rng)
        cases.append((x, u, status_of(pattern, n, rng), n, om, v, (b + len(appended)) % 3 != 0, state))
    kept = [int(np.count_nonzero(c[2][:c[3]])) for c in cases]
    if appended == "none":
        new_counts, max_total = None, S_EDGE
    elif appended == "some":
        new_counts, max_total = [17 + b for b in range(len(ns))], S_EDGE
    elif appended == "clamped":                                  # more than max_total - kept: the budget cuts them
        new_counts, max_total = [40] * len(ns), min(S_EDGE, max(kept) + 5)
    else:                                                        # "full": kept == max_total in stream 0 (more in none): nothing fits
        new_counts, max_total = [9] * len(ns), kept[0]
    got, rec, want = run_stage(ctx, ofk, cases, SET, new_counts, max_total)
    compare_stage(got, rec, want, (case, tuple(ns), max_total))
    for b, (_, _, count, _) in enumerate(want):
        extra = count - kept[b]
        if appended == "clamped":
            assert extra == max(0, min(40, max_total - kept[b])), (case, b)
        if appended == "full" and b == 0:
            assert extra == 0, case
        if extra > 0:
            assert not got["nobs"][b, kept[b]:count].any() and not got["rho"][b, kept[b]:count].any(), (case, b)
    return [w[1] for w in want]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_step_kernel_edges(ctx, ofk, pattern):
    """Every count under one status pattern, the four kinds of appends in turn, three streams per call."""
    groups = [COUNTS[0:3], COUNTS[3:6], COUNTS[6:9], (COUNTS[9], COUNTS[4], COUNTS[7])]
    solved_maps = 0
    for g, ns in enumerate(groups):
        recs = check_step(ctx, ofk, ns, pattern, ("none", "some", "clamped", "full")[g], (pattern, g))
        solved_maps += sum(r[3] == 0 for r in recs)
    if pattern in ("all", "random"):
        assert solved_maps >= 4, solved_maps                     # the comparison of v_map and C_map is not one of zeros
    print("largest deviation of v_map / C_map so far, in units of the slot group's scale:", DEV[0])


def test_three_streams_of_different_counts(ctx, ofk):
    for ns in ((1030, 0, 257), (1, 513, 64), (300, 300, 299)):
        recs = check_step(ctx, ofk, ns, "random", "clamped", ("mixed", ns))
        assert sum(r[3] == 0 for r in recs) >= 1, ns
    print("largest deviation of v_map / C_map so far, in units of the slot group's scale:", DEV[0])


# ------------------------------------------------------------------------------------------------ (c) every skip and reset path
def path_case(rng, S=80):
    x = rng.uniform(-1.0, 1.0, (S, 2)) * [T.W2, T.H2]
    v, om = er.V.copy(), er.OM.copy()
    rho_true = rng.uniform(0.5, 1.4, S)
    u = er.flow(x, v, om, rho_true) + rng.normal(0, 0.2 * er.SIGMA_FLOW, (S, 2))
    state = dict(rho=rho_true * (1.0 + rng.normal(0, 0.002, S)), var=(0.01 * rho_true) ** 2, nobs=np.full(S, 5, np.int32))
    b = v[None, :2] - v[2] * x
    across = np.stack([-b[:, 1], b[:, 0]], 1) / np.linalg.norm(b, axis=1)[:, None]
    x[0] = v[:2] / v[2] + 1e-5; u[0] = er.flow(x[0:1], v, om, [1.0])[0]               # next to the focus of expansion: |b| < b_min
    u[1] += 10 * er.SIGMA_FLOW * across[1]                       # across the epipolar line: the cross-flow gate
    state["rho"][2] *= 1.5                                       # the innovation gate
    for k in (3, 4):                                             # rows without a depth: one is initialised, one sees z <= 0
        state["rho"][k] = 0.0; state["var"][k] = 0.0; state["nobs"][k] = 0
    u[4] = er.flow(x[4:5], v, om, [-0.8])[0]
    x[5] = np.nan; u[6] = np.inf; x[7] = [np.inf, 0.1]           # no number in a point
    st = np.ones(S, np.uint8); st[8] = 0; st[40:44] = 0
    return x, u, st, v, om, state


def test_every_skip_and_reset_path(ctx, ofk):
    rng = np.random.default_rng(11)
    x, u, st, v, om, state = path_case(rng)
    S = len(x)
    v_fast = v.copy(); v_fast[2] = -0.95 / 0.5                   # g = 1 + rho v_z < 0.1 for every rho > 0.5: the rows are reset
    variants = [("default", SET, v, True), ("update-0", dict(SET, update=0), v, True), ("gate-0", dict(SET, gate=0.0), v, True),
                ("unsolved", dict(SET, q=1e-6), v, False), ("g-small", SET, v_fast, True), ("v-nan", SET, np.array([0.02, -0.015, np.nan]), True)]
    seen = {}
    for name, s, vv, solved in variants:                         # a launch has one setting: each variant in a launch of its own
        got, rec, want = run_stage(ctx, ofk, [(x, u, st, S - 2, om, vv, solved, state)], s, [3], S)
        compare_stage(got, rec, want, name)
        seen[name] = want[0][1]
    d = seen["default"]
    # |b| short and two points that are no numbers; the cross-flow gate (the infinite flow too); the innovation gate; one row
    # initialised, the z <= 0 one not; the two points whose prediction is no number reset
    assert d[7] >= 3 and d[8] >= 2 and d[9] >= 1 and d[6] == 1 and d[20] >= 2 and d[5] >= 50, d
    assert seen["update-0"][5] == 0 and seen["update-0"][6] == 1 and seen["update-0"][9] == 0, seen["update-0"]
    assert seen["gate-0"][8] == 0 and seen["gate-0"][9] == 0 and seen["gate-0"][5] > d[5], seen["gate-0"]
    assert not seen["unsolved"][5:10].any() and seen["unsolved"][19] == 0 and seen["unsolved"][20] == 0, seen["unsolved"]
    assert seen["g-small"][20] >= 60, seen["g-small"]
    assert not seen["v-nan"][5:10].any() and seen["v-nan"][19] == 1 and seen["v-nan"][20] >= 60, seen["v-nan"]


def test_python_stage_entries(pkg, ofk):
    """velocity_node.track_depth_step and simulation.track_depth_step: the restatement's rows through the facade."""
    from of_amd import simulation, velocity_node
    rng = np.random.default_rng(5)
    x, u, st, v, om, state = path_case(rng)
    n = len(x)
    want, wrec, count, _ = T.step(state, x, u, st, n, om, v, True, SET, new_count=4, max_total=n)
    for mod in (velocity_node, simulation):
        got, rec = mod.track_depth_step(x, u, om, v, state=state, status=st, new_count=4, sigma_flow=SET["sigma_flow"], b_min=SET["b_min"], q=SET["q"])
        assert count == len(got["rho"]) and all(np.array_equal(bits(got[k]), bits(want[k][:count])) for k in KEYS), mod.__name__
        same_record(rec, wrec, mod.__name__)


# ------------------------------------------------------------------------------------------------ (d)-(h) streams
H, W, NF, B = 128, 160, 9, 2
MOTION = dict(v=(0.012, -0.008, 0.004), omega=(0.002, -0.001, 0.004), d=1.0)
MC, MF, RADIUS = 120, 100, 5
MC_BEGIN = 100                                                  # ofk_stream_step's streams begin with fewer corners than their steps may hold: rows are appended
_frames = {}


def frames_of(pkg):
    if "f" not in _frames:
        from of_amd import synth
        seqs = [synth.render_sequence(H, W, 60 + b, NF, margin=64, **MOTION) for b in range(B)]
        _frames["f"] = (np.stack([s[0] for s in seqs]), seqs[0][1])
    return _frames["f"]


def stream_cfg(**kw):
    from of_amd.pipeline import PipelineConfig
    return PipelineConfig(max_corners=MC, quality=0.01, min_distance=4, block_size=5, win=15, max_level=2, max_count=20, eps=0.03, min_eig_thr=1e-4, **kw)


def sensor_rows(ofk, info, n=B):
    return ofk.make_sensors(n, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"], v_prior=info["v"])


class Follower:
    """The restated depths of a context's streams, advanced with what the calls hand back and compared after every call."""

    def __init__(self, ctx, S, s=T.DEFAULTS):
        self.ctx, self.S, self.s = ctx, S, s

    def start(self, tracks, counts):
        """The streams have these tracks and no depths: the device zeroes its rows in front of the next step."""
        self.B = len(counts)
        self.st = [T.empty(self.S) for _ in range(self.B)]
        self.pos = [tracks[b, :counts[b]].copy() for b in range(self.B)]
        self.rec = [None] * self.B
        return self

    def replaced(self, b, new_pts):
        new_pts = np.asarray(new_pts, np.float32).reshape(-1, 2)
        for k in KEYS:
            self.st[b][k][:len(new_pts)] = 0
        self.pos[b] = new_pts.copy()

    def compare(self, tag):
        d = self.ctx.track_depth_download(self.B, self.S)
        for b in range(self.B):
            n = len(self.pos[b])
            for k in KEYS:
                assert np.array_equal(bits(d[k][b, :n]), bits(self.st[b][k][:n])), (tag, b, k, np.flatnonzero(bits(d[k][b, :n]) != bits(self.st[b][k][:n]))[:4])
            if self.rec[b] is not None:
                same_record(d["rec"][b], self.rec[b], (tag, b))
        return d

    def step(self, rec, tracks, counts, max_total, sensors, fused, tag, held=False, omega=None, ideal=None):
        if held:                                                 # a held step launches nothing (a replace in front of it has happened)
            return self.compare((tag, "held"))
        nxt, keep = self.ctx.stream_last_points(self.S)
        for b in range(self.B):
            n_old = len(self.pos[b])
            prev = self.pos[b] if ideal is None else ideal[0][b, :n_old]
            new = nxt[b, :n_old] if ideal is None else ideal[1][b, :n_old]
            sr = sensors[b]
            x = (new.astype(np.float64) - [sr[20], sr[21]]) * sr[19]
            u = (new.astype(np.float64) - prev.astype(np.float64)) * sr[19]
            kept = int(np.count_nonzero(keep[b, :n_old]))
            solved = rec[b, 15] != 0 if fused else rec[b, 4] >= 3
            self.st[b], self.rec[b], count, _ = T.step(self.st[b], x, u, keep[b, :n_old], n_old, sr[4:7] if omega is None else omega[b], rec[b, 0:3],
                                                       bool(solved), self.s, new_count=int(counts[b]) - kept, max_total=max_total, scale=sr[19])
            assert count == counts[b], (tag, b, count, counts[b])
            self.pos[b] = tracks[b, :counts[b]].copy()
        return self.compare(tag)


def jpeg_of(batch):
    from PIL import Image
    res = []
    for img in batch:
        buf = _io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=92)
        res.append(buf.getvalue())
    return res


def run_plain(pkg, ofk, depth, jpeg_step=None, on_from=1):
    """ofk_stream_step over the 8 steps; the streams begin with MC_BEGIN corners and re-detect up to MC whenever they hold fewer; depth:
    the setting is on (from step on_from on).  jpeg_step: that step's frames arrive as JPEG streams.  -> everything the calls returned."""
    frames, info = frames_of(pkg)
    cfg, sensors = stream_cfg(), sensor_rows(ofk, info)
    ctx = ofk.Context(0, W, H, B, MC, cfg.max_level)
    out, fol, solved_maps, appended = [], None, 0, 0
    try:
        ctx.set_track_table(ofk.track_table_setting())
        tracks, counts = ctx.stream_begin(frames[:, 0], dataclasses.replace(cfg, max_corners=MC_BEGIN).to_params())
        out.append((tracks.copy(), counts.copy()))
        for t in range(1, NF):
            if depth and t == on_from:
                ctx.set_track_depth(ofk.track_depth_setting())
                fol = Follower(ctx, MC).start(tracks, counts)
            before = counts.copy()
            if t == jpeg_step:
                rec, tracks, counts = ctx.stream_step_jpeg(jpeg_of(frames[:, t]), sensors, cfg.to_params(), MC, RADIUS)
            else:
                rec, tracks, counts = ctx.stream_step(frames[:, t], sensors, cfg.to_params(), MC, RADIUS)
            out.append((rec.copy(), tracks.copy(), counts.copy(), ctx.track_table_download(B, MC)))
            if fol:
                d = fol.step(rec, tracks, counts, MC, sensors, False, ("plain", t))
                solved_maps += int((d["rec"][:, 3] == 0).sum())
                appended += int((counts > before).sum())
                print("plain step", t, "counts", before, "->", counts, "mature rows", d["rec"][:, 4], "map flags", d["rec"][:, 3])
        if fol and on_from == 1 and jpeg_step is None:
            assert solved_maps >= B and appended >= 1, (solved_maps, appended)       # the map solve ran on mature rows; rows were appended
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


def run_fused(pkg, ofk, depth, kind):
    """ofk_stream_step_fused on the sensors, no filter.  kind: "robust" (the robust solve drops its outliers from the tracks) |
    "zones" (and the exclusion zones grow from them) | "replace" (streams with few tracks replace them in front of LK) | "hold"
    (one stream; steps 3 and 4 are not solved and held) | "epipolar" | "camera" | "imu"."""
    from of_amd.pipeline import CameraModel, FusionConfig
    frames, info = frames_of(pkg)
    nb = 1 if kind == "hold" else B
    frames = frames[:nb]
    robust = kind in ("robust", "zones")
    cfg = stream_cfg(**(dict(robust="tukey", robust_drop=True) if robust else {}))
    sensors = sensor_rows(ofk, info, nb)
    fusion = FusionConfig(use_imu=kind == "imu", redetect_replace=kind == "replace", hold_on_skip=kind == "hold")
    cam = CameraModel(fx=160.0, fy=160.0, cx=80.0, cy=64.0, k=(-0.1, 0.01, 0, 0)) if kind == "camera" else None
    if cam is not None:
        sensors[:, 19:22] = cam.sensor_slots()
    mf = MC - 10 if kind == "replace" else MF
    ctx = ofk.Context(0, W, H, nb, MC, cfg.max_level)
    out, solved_maps, events = [], 0, 0
    try:
        if robust:
            ctx.set_robust(cfg.robust_setting())
        if kind == "zones":
            ctx.set_zones(ofk.zones_setting(link=24, min_members=2, radius=8, ttl=4))
        if kind == "epipolar":
            ctx.set_epipolar(ofk.epipolar_setting(sigma_max=np.inf))
        if cam is not None:
            ctx.set_camera(cam.setting())
        ctx.imu_reset(nb)
        ctx.set_track_table(ofk.track_table_setting())
        if depth:
            ctx.set_track_depth(ofk.track_depth_setting())
        tracks, counts = ctx.stream_begin(frames[:, 0], cfg.to_params())
        fol = Follower(ctx, MC).start(tracks, counts) if depth else None
        prev_frame = 0
        for t in range(1, NF):
            fs = fusion.to_struct()
            if kind == "hold" and t in (3, 4):
                fs.min_solve = 10 ** 6                           # more points than there are: not solved
            if kind == "replace" and fol:
                for b in range(nb):                              # k_redetect_limits' rule, the detection of the reference loop
                    budget = MC - len(fol.pos[b])
                    if len(fol.pos[b]) <= mf and budget > 0:
                        g_prev = io.gray_bgr8(frames[b, prev_frame])
                        fol.replaced(b, io.good_features(g_prev, budget, cfg.quality, cfg.min_distance, cfg.block_size).reshape(-1, 2))
                        events += 1
            rec, fused, tracks, counts = ctx.stream_step_fused(frames[:, t], sensors, cfg.to_params(), fs, mf, RADIUS)
            hold = kind == "hold" and rec[0, 15] == 0
            out.append((rec.copy(), fused.copy(), tracks.copy(), counts.copy(), ctx.track_table_download(nb, MC)) +
                       ((ctx.zones_download(nb),) if kind == "zones" else ()))
            if fol:
                omega = ctx.imu_state(nb)[0][:, 18:21] if kind == "imu" else None
                ideal = ctx.camera_download(nb) if cam is not None else None
                d = fol.step(rec, tracks, counts, MC, sensors, True, (kind, t), held=hold, omega=omega, ideal=ideal)
                solved_maps += int((d["rec"][:, 3] == 0).sum())
                events += int(hold)
                if robust:
                    events += int(sum(rec[b, 13] - (rec[b, 11]) for b in range(nb)))       # tracked by LK, not kept by the solve
            if not hold:
                prev_frame = t
        if fol:
            print(kind, "map solves on mature rows:", solved_maps, "events (rows dropped by the solve / replacements / held steps):", events)
            if kind != "replace":                                # a replaced stream starts over: its rows may never mature
                assert solved_maps >= 1, (kind, "no map solve on mature rows")
            if kind in ("robust", "zones", "replace", "hold"):    # the case is the one it is named after
                assert events >= (2 if kind == "hold" else 1), (kind, events)
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("kind", ["robust", "zones"])
def test_stream_step_fused_with_robust_drop(pkg, ofk, kind):
    same(run_fused(pkg, ofk, True, kind), run_fused(pkg, ofk, False, kind), (kind, "on against off"))


def test_stream_replace_redetection(pkg, ofk):
    run_fused(pkg, ofk, True, "replace")


def test_held_steps_leave_the_depths(pkg, ofk):
    run_fused(pkg, ofk, True, "hold")


@pytest.mark.parametrize("kind", ["epipolar", "camera", "imu"])
def test_composition(pkg, ofk, kind):
    run_fused(pkg, ofk, True, kind)


def test_refusals(pkg, ofk):
    from of_amd.pipeline import FusionConfig
    frames, info = frames_of(pkg)
    cfg, sensors = stream_cfg(), sensor_rows(ofk, info)
    ctx = ofk.Context(0, W, H, B, MC, cfg.max_level)
    try:
        ctx.imu_reset(B)
        ctx.set_track_depth(ofk.track_depth_setting())
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
            assert e.value.code == ofk.E_INVALID and "ofk_set_track_depth" in str(e.value), str(e.value)
        with pytest.raises(ofk.OfkError):                          # nothing was launched: no depths yet
            ctx.track_depth_download(B)
        rec, fused, tracks2, counts2 = ctx.stream_step_fused(frames[:, 1], sensors, cfg.to_params(), plain, MF, RADIUS)     # the stream goes on
        assert ctx.track_depth_download(B)["rec"][:, 19].all() and rec[:, 15].all()
    finally:
        ctx.close()


def test_depth_reset_loads_rows(pkg, ofk):
    """ofk_track_depth_reset: a hint from outside is a row like any other in the next step."""
    frames, info = frames_of(pkg)
    cfg, sensors = stream_cfg(), sensor_rows(ofk, info)
    ctx = ofk.Context(0, W, H, B, MC, cfg.max_level)
    try:
        ctx.set_track_table(ofk.track_table_setting()); ctx.set_track_depth(ofk.track_depth_setting())
        tracks, counts = ctx.stream_begin(frames[:, 0], cfg.to_params())
        fol = Follower(ctx, MC).start(tracks, counts)
        n = int(counts[1])
        hint = dict(rho=np.full(n, 1.0), var=np.full(n, 0.04), nobs=np.full(n, 3, np.int32))       # the plane at d = 1, 20 %
        ctx.track_depth_reset(1, hint["rho"], hint["var"], hint["nobs"])
        for k in KEYS:
            fol.st[1][k][:n] = hint[k]
        fol.compare("reset")
        rec, tracks, counts = ctx.stream_step(frames[:, 1], sensors, cfg.to_params(), MF, RADIUS)
        d = fol.step(rec, tracks, counts, MC, sensors, False, "after reset")
        assert d["rec"][1, 3] == 0 and d["rec"][1, 4] >= 8 and d["rec"][0, 3] == 1        # the hinted stream solves its map at once
        with pytest.raises(ofk.OfkError):
            ctx.track_depth_reset(B, [1.0], [0.1], [1])
        with pytest.raises(ofk.OfkError):
            ctx.track_depth_reset(0, [1.0], [0.1], [-1])
    finally:
        ctx.close()


def plane_share(rho, var, nobs, pts, sr, dist, nrm):
    """(mature rows, of those the share within 3 sqrt(var) of the plane's inverse depth, their median relative depth error)."""
    mature = (nobs >= 3) & (rho > 0) & (var <= (0.25 * rho) ** 2)
    x = (np.asarray(pts, np.float64) - [sr[20], sr[21]]) * sr[19]
    want = er.plane_rho(x, dist, nrm)
    inside = np.abs(rho - want)[mature] <= 3.0 * np.sqrt(var[mature])
    return int(mature.sum()), float(inside.mean()), float(np.median(np.abs(rho - want)[mature] / want[mature]))


def test_plane_sequence_through_the_device_chain(pkg, ofk):
    """8 steps over a plane.  The CPU run first: the same frames through the C oracle chain (tests/stream_oracle.NodeLoop) and the
    restatement give the share of mature rows whose depth lies within 3 sqrt(var) of the plane's inverse depth.  The device chain
    reaches that share (its state is the restatement's after every step, and the map solve is solved at the end)."""
    import stream_oracle as so
    frames, info = frames_of(pkg)
    cfg, sensors = stream_cfg(), sensor_rows(ofk, info)
    v, om = np.asarray(info["v"], np.float64), np.asarray(info["omega"], np.float64)
    Ai = np.linalg.inv(np.eye(3) + np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]]))
    nrm, dist = np.asarray(info["n"], np.float64), float(info["d"])
    for _ in range(NF - 1):                                      # the plane in the axes of the last frame: P+ = A P + v
        n2 = Ai.T @ nrm
        dist = (dist + nrm @ (Ai @ v)) / np.linalg.norm(n2); nrm = n2 / np.linalg.norm(n2)
    cpu = []
    for b in range(B):
        loop, st = so.NodeLoop(frames[b, 0], cfg, 0, RADIUS), T.empty(MC)
        for t in range(1, NF):
            o = loop.step(frames[b, t], sensors[b])
            new, old = np.asarray(o["new"], np.float64).reshape(-1, 2), np.asarray(o["old"], np.float64).reshape(-1, 2)
            st, _, count, _ = T.step(st, (new - [sensors[b, 20], sensors[b, 21]]) * sensors[b, 19], (new - old) * sensors[b, 19], np.asarray(o["keep"]).ravel(),
                                     len(new), sensors[b, 4:7], np.zeros(3) if o["v"] is None else o["v"], o["v"] is not None, T.DEFAULTS, new_count=0,
                                     max_total=MC, scale=sensors[b, 19])
        cpu.append(plane_share(st["rho"][:count], st["var"][:count], st["nobs"][:count], o["tracks"], sensors[b], dist, nrm))
        assert cpu[b][0] >= 8, cpu[b]
    ctx = ofk.Context(0, W, H, B, MC, cfg.max_level)
    try:
        ctx.set_track_table(ofk.track_table_setting()); ctx.set_track_depth(ofk.track_depth_setting())
        tracks, counts = ctx.stream_begin(frames[:, 0], cfg.to_params())
        fol = Follower(ctx, MC).start(tracks, counts)
        for t in range(1, NF):
            rec, tracks, counts = ctx.stream_step(frames[:, t], sensors, cfg.to_params(), 0, RADIUS)
            d = fol.step(rec, tracks, counts, MC, sensors, False, ("plane", t))
        for b in range(B):
            n = int(counts[b])
            got = plane_share(d["rho"][b, :n], d["var"][b, :n], d["nobs"][b, :n], tracks[b, :n], sensors[b], dist, nrm)
            assert d["rec"][b, 3] == 0 and d["rec"][b, 4] >= 8, (b, d["rec"][b])
            assert got[0] >= cpu[b][0] and got[1] >= cpu[b][1], (b, got, cpu[b])
            vm = d["rec"][b, 0:3]
            print("stream", b, "mature rows, share within 3 sigma of the plane, median relative depth error: device", got, "CPU chain", cpu[b],
                  "v_map's relative error", round(float(np.linalg.norm(vm - v) / np.linalg.norm(v)), 4),
                  "the record's", round(float(np.linalg.norm(rec[b, 0:3] - v) / np.linalg.norm(v)), 4))
    finally:
        ctx.close()
