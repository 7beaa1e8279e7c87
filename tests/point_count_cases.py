"""Inputs and references of the point-count tests (tests/test_gpu_point_counts.py, tests/test_gpu_stream_counts.py and their CPU
companion tests/test_point_count_cases.py): the tracking chain past 256 and 512 points per image, and at none.  Every kernel of
that chain walks an image's points in passes of 256 threads; the cases here make the second and third pass, the partly filled last
pass and the empty image happen.  Everything is computed once per process and handed out unchanged.  Test infrastructure only; the
product never imports it.

points()        S = 1030 points of the gate tests' scene: corners in the even slots, random and border positions in the odd ones.
COUNTS          the point counts every stage entry runs at (chunk edges, wave edges, all residues mod 4, one, none).
gate_case()     track_gate_reference.gated on the 1030 points, and prefix() = the same for the first c of them.
lk_case()       lk_seed_reference.lk_pyr on the 1030 points under the cv2 flags.
stream_run()    the restated stream loop (stream_oracle.NodeLoop) over four streams under a per-step plan of (max_corners,
                min_features), the exact-boundary steps derived from the loop's own trajectory.
module_run()    stream_oracle.oracle_of_module for the replace re-detection.
pair_scenes()   the moving-object scene of robust_reference.scene at 240 x 320, 600 corners, for the robust solve past 512 points."""
import dataclasses

import numpy as np

from oracle import image_oracle as io
import lk_seed_reference as R  # tests/lk_seed_reference.py
import track_gate_reference as G  # tests/track_gate_reference.py
from point_stage_helpers import bits  # tests/point_stage_helpers.py
import robust_reference as rr  # tests/robust_reference.py
import robust_stream_oracle as rso  # tests/robust_stream_oracle.py
from stream_oracle import NodeLoop, oracle_of_module, track
from test_gpu_track_gate import H, W, MOTION, LK, STREAM_MOTION, VARIANTS  # the gate tests' scene and settings

S = 1030
COUNTS = (1030, 1024, 769, 768, 513, 512, 511, 258, 257, 256, 255, 129, 65, 64, 63, 7, 6, 5, 1, 0)
GROUPS = tuple(COUNTS[i:i + 4] for i in range(0, len(COUNTS), 4))           # four images per call of the session context
CHUNKS = ((256, 512), (512, 768), (768, 1024))                              # passes 1, 2 and 3 of a 256-thread workgroup
SENTINEL = np.float32(-12345.678)                                           # what lies beyond an image's count
FORWARD_SHIFT = np.array([3, -2], np.float32)                               # the seeded forward pass starts at points + this
POINT_SEED = 1056          # of the random slots; chosen on the reference so that every chunk of every gate case meets the CPU companion's limits
_cache = {}


def differing(got, want):
    """Indices of the entries (rows) of two arrays that differ in a bit."""
    d = bits(got) != bits(want)
    return np.flatnonzero(d.reshape(len(d), -1).any(1)) if len(d) else np.zeros(0, np.int64)


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def synth():
    from __graft_entry__ import load_package
    load_package()
    from of_amd import synth as s
    return s


# ------------------------------------------------------------------------------------------------ section 1: the stage entries
def scene():
    def make():
        pair = synth().render_pair(H, W, 5, margin=64, **MOTION)
        return dict(pair=pair, g0=io.gray_bgr8(pair["prev"]), g1=io.gray_bgr8(pair["next"]))
    return cached("scene", make)


def points():
    """[S,2] f32.  Even slots: good_features(g0, 2048, 0.0005, 2, 5).  Odd slots: the border points of tests/test_gpu_lk_seed.py
    ::points, then uniformly random positions in [-3, w+3) x [-3, h+3).  So every 256-chunk holds tracked, lost and far points."""
    def make():
        g0 = scene()["g0"]
        c = io.good_features(g0, 2048, 0.0005, 2, 5).reshape(-1, 2)
        assert len(c) == 2048, len(c)
        h, w, win = H, W, 15
        edge = np.array([(-2.5, 9.0), (0.3, 0.2), (w - 1.2, 4.5), (w + 1.0, h / 2), (w / 2, -1.5), (w / 2, 0.4), (w / 2, h - 0.6), (w / 3, h + 2.0),
                         (1.5, h - 1.5), (w - 1.5, h - 1.5), (w - 0.5, 0.5), (win / 2.0, win / 2.0)], np.float32)
        rng = np.random.default_rng(POINT_SEED)
        odd = S // 2
        r = np.stack([rng.uniform(-3, w + 3, odd), rng.uniform(-3, h + 3, odd)], 1).astype(np.float32)
        r[np.arange(len(edge)) * (odd // len(edge))] = edge                 # the border points spread over all chunks
        p = np.zeros((S, 2), np.float32)
        p[0::2] = c[:S - odd]; p[1::2] = r
        p.setflags(write=False)
        return p
    return cached("points", make)


def forward_seed():
    return (points() + FORWARD_SHIFT).astype(np.float32)


# window, variant, forward pass seeded, err cap
GATE_CASES = [(win, var, False, False) for win in (5, 15, 21) for var in ("plain-L2", "seeded-L0")]
GATE_CASES += [(15, "plain-L2", False, True), (5, "seeded-L0", False, True), (21, "plain-L2", False, True),
               (21, "plain-L2", True, False), (15, "seeded-L0", True, False)]


def gate_id(case):
    win, var, fseed, cap = case
    return f"win{win}-{var}" + ("-forward-seeded" if fseed else "") + ("-errcap" if cap else "")


def gate_case(win, var, fseed=False, cap=False, fb_thr=0.5):
    """dict(gate, seed, flags, ref): the setting and track_gate_reference.gated on all S points.  The err cap is the median err of
    the forward-tracked points, so about half of them fall to it."""
    def make():
        s = scene()
        seed = forward_seed() if fseed else None
        flags = R.USE_INITIAL_FLOW if fseed else 0
        gate = G.setting(fb_thr=fb_thr, **VARIANTS[var])
        if cap:
            base = gate_case(win, var, fseed, False, fb_thr)["ref"]
            gate["err_max"] = float(np.median(base["err"][base["st_f"] == 1]))
        ref = G.gated(s["g0"], s["g1"], points(), win, gate=gate, seed=seed, flags=flags, **LK)
        return dict(gate=gate, seed=seed, flags=flags, ref=ref)
    return cached(("gate", win, var, fseed, cap, fb_thr), make)


def gate_masks(r, gate):
    """(lost in the backward pass, far, capped, kept) of a gated() result, by the rules of ofk.h."""
    st_f, st_b, keep = r["st_f"] == 1, r["st_b"] == 1, r["status"] == 1
    with np.errstate(all="ignore"):
        far = st_f & st_b & ~(r["fb2"] <= np.float32(gate["fb_thr"] * gate["fb_thr"])) if gate["fb"] != "off" else np.zeros(len(keep), bool)
    return st_f & ~st_b, far, st_f & st_b & ~far & ~keep, keep


def prefix(r, gate, c):
    """gated() of the first c points from gated() of all of them: LK and the gate treat every point on its own (the CPU companion
    checks this against a direct call), only the four counts are per image."""
    out = {k: r[k][:c] for k in ("next", "status", "st_f", "err", "back", "st_b", "fb2", "keep")}
    lost, far, capped, _ = gate_masks(out, gate)
    out["stats"] = np.array([(out["st_f"] == 1).sum(), lost.sum(), far.sum(), capped.sum()], np.int32)
    return out


def threshold_edges():
    """Three (index, d, thr_keep, thr_far): kept points of chunks 0, 1 and 2 of the win-15 plain-L2 case whose squared distance d is
    met exactly by float32(thr_keep^2), while float32(thr_far^2) is the next float32 below d (ofk.h: squared in double, rounded once)."""
    def search(d):
        d = np.float32(d)
        t = float(np.sqrt(np.float64(d)))
        for _ in range(64):                                     # the double whose square rounds to d, walking from sqrt(d)
            q = np.float32(t * t)
            if q == d:
                return t
            t = float(np.nextafter(t, np.inf if q < d else -np.inf))
        return None

    def make():
        ref = gate_case(15, "plain-L2")["ref"]
        found = []
        for lo, hi in ((0, 256), (256, 512), (512, 768)):
            kept = np.flatnonzero(ref["keep"][lo:hi]) + lo
            mid = np.median(ref["fb2"][kept])                    # a threshold in the middle of the kept points' distances splits them
            for i in kept[np.argsort(np.abs(ref["fb2"][kept] - mid), kind="stable")]:
                d = ref["fb2"][i]
                if not d > np.float32(1e-6):
                    continue
                below = np.nextafter(d, np.float32(-np.inf), dtype=np.float32)
                a, b = search(d), search(below)
                if a is not None and b is not None:
                    found.append((int(i), d, a, b))
                    break
        return found
    return cached("edges", make)


LK_FLAG_CASES = [(flags, L) for flags in (R.USE_INITIAL_FLOW, R.GET_MIN_EIGENVALS, R.USE_INITIAL_FLOW | R.GET_MIN_EIGENVALS) for L in (0, 2)]
LK_PARAMS = dict(max_count=LK["max_count"], eps=LK["eps"], min_eig_thr=LK["min_eig_thr"])


def lk_case(flags, L, win=15):
    """lk_seed_reference.lk_pyr on all S points -> (next [S,2], status [S], err [S])."""
    def make():
        s = scene()
        seed = forward_seed() if flags & R.USE_INITIAL_FLOW else None
        n, st, e = R.lk_pyr(s["g0"], s["g1"], points(), win, L, seed=seed, flags=flags, **LK_PARAMS)
        return n.reshape(-1, 2), st.ravel(), e.ravel()
    return cached(("lk", flags, L, win), make)


# ------------------------------------------------------------------------------------------------ section 2: the stream lifecycle
NF, B_STREAMS = 8, 4
BLANK_STREAM, BLANK_FRAMES = 1, (3, 4)
# (max_corners, min_features) -> the rest of the detector's setting; mask_radius 6, block_size 5 everywhere
RUNS = {(600, 590): dict(quality=0.0005, min_distance=2), (600, 520): dict(quality=0.0005, min_distance=2),
        (520, 512): dict(quality=0.0005, min_distance=2), (300, 256): dict(quality=0.001, min_distance=3)}
MASK_RADIUS = 6
ROBUST = dict(rso.SETTING)                                      # TUKEY, K = 64, 5 rounds


def stream_frames(blank=False):
    """([B,NF,h,w,3] frames, info).  blank: frames 3 and 4 of stream 1 are a uniform 128 (a drone over textureless ground)."""
    def make():
        seqs = [synth().render_sequence(H, W, 40 + b, NF, margin=160, **STREAM_MOTION) for b in range(B_STREAMS)]
        frames = np.stack([s[0] for s in seqs])
        if blank:
            frames = frames.copy()
            for t in BLANK_FRAMES:
                frames[BLANK_STREAM, t] = 128
        frames.setflags(write=False)
        return frames, seqs[0][1]
    return cached(("frames", blank), make)


def sensor_rows(info, B=B_STREAMS):
    """The [B,28] sensor records of a rendered scene, its true velocity as the prior."""
    from of_amd import ofk
    return ofk.make_sensors(B, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"], v_prior=info["v"])


def stream_cfg(max_corners, variant=None, drop=False):
    from of_amd.pipeline import PipelineConfig
    base = next(v for k, v in RUNS.items() if k[0] == max_corners)
    cfg = PipelineConfig(max_corners=max_corners, block_size=5, win=15, max_level=LK["max_level"], max_count=LK["max_count"], eps=LK["eps"],
                         min_eig_thr=LK["min_eig_thr"], **base)
    if variant == "gate":
        g = VARIANTS["seeded-L0"]
        cfg.fb_check, cfg.fb_thr, cfg.fb_level = g["fb"], 0.5, g["fb_level"]
    if variant in ("robust", "robust-fused"):
        cfg.robust = "tukey"; cfg.robust_c = ROBUST["c"]; cfg.robust_iters = ROBUST["iters"]; cfg.robust_hypotheses = ROBUST["hypotheses"]
        cfg.robust_seed = ROBUST["seed"]; cfg.robust_drop = bool(drop)
    if variant == "seed":
        cfg.lk_seed = "model"; cfg.seed_gain = 1.0
    return cfg


def kf3_fusion():
    from of_amd.pipeline import FusionConfig, FilterModel
    return FusionConfig(use_imu=False, filter=True, z_sign=1.0, z_source=1, model=FilterModel.kf3())


# The runs whose last two steps land on a chunk boundary and one above it.  The (600, 590) run never tracks fewer than 512 points and
# a step only ever adds to the tracked points, so it cannot land on 512: it is the run of three full chunks and a filled budget.
LANDING = {(600, 520): 512, (520, 512): 512, (300, 256): 256}


def plan_steps(kind, max_corners, min_features):
    """What each of the NF - 1 steps is asked for: the run's (max_corners, min_features), and for the "edges" runs of LANDING in the
    last two steps a landing on the boundary and on the count one above it (see stream_run)."""
    plan = [dict(max_corners=max_corners, min_features=min_features, land=None) for _ in range(NF - 1)]
    edge = LANDING.get((max_corners, min_features))
    if kind == "edges" and edge:
        plan[-2]["land"] = edge; plan[-1]["land"] = edge + 1
    return plan


def stream_run(kind, max_corners, min_features, radius=MASK_RADIUS, variant=None, drop=False, seeds=None):
    """The restated loop over the four streams.  kind "edges": textured frames; "zero": stream 1 loses its texture in two frames.
    variant: None (plain step) | "kf3" (step_fused with the three-state filter) | "gate" | "robust" (plain step) | "robust-fused"
    (step_fused on the sensors, no filter) | "seed".
    seeds: for "seed", a function (old [B,mc,2], counts [B]) -> start positions [B,mc,2] (the device's predictor, as in
    tests/test_gpu_seed_pipeline.py).

    A step that has to LAND on a count (plan "land") tracks the reference's current tracks once to learn n_tracked, then asks for
    max_corners = land + n_old - n_tracked and min_features = max_corners for every stream whose n_tracked is below `land`: the stream
    re-detects with a budget of max_corners - n_old corners, and n_tracked + appended == land when the detector fills the budget.
    The device is given the same two numbers per step, taken from stream 0, the only stream the landing is asserted for.
    kind "zero": one min_features serves the whole batch (ofk_stream_step), so a stream cannot be kept from re-detecting by a value
    of its own.  Instead min_features of a step is the median track count of the three textured streams before it: the two with
    fewer tracks re-detect with a small budget, the one with more does not (budget 0), and the emptied stream asks for max_corners
    - all in one call.
    -> dict(first, steps [t][b] = NodeLoop.step's dict (plus "gate": the gate's full result; "valid": who the robust solve was given), asked [t] = (max_corners, min_features),
    cfg, sensors [B,28])."""
    def make():
        frames, info = stream_frames(kind == "zero")
        sens = sensor_rows(info)
        cfg = stream_cfg(max_corners, variant, drop)
        fused = variant == "kf3"
        logs = [[] for _ in range(B_STREAMS)]
        loops = []
        for b in range(B_STREAMS):
            kw = {}
            if variant == "gate":
                kw["lk"] = G.gated_lk(cfg, G.setting(fb_thr=0.5, **VARIANTS["seeded-L0"]), logs[b])
            if variant in ("robust", "robust-fused"):
                inner = rso.robust_solver(b, drop, variant == "robust-fused", ROBUST)
                kw["solve"] = lambda x, u, ok, d, nrm, om, inner=inner: dict(inner(x, u, ok, d, nrm, om), valid=ok.copy())     # + who was tracked
            if fused:
                kw["model"] = kf3_fusion().model
            loops.append(NodeLoop(frames[b, 0], cfg, min_features, radius, **kw))
        first = [l.tracks.copy() for l in loops]
        steps, asked = [], []
        for t, want in enumerate(plan_steps(kind, max_corners, min_features), start=1):
            mc, mf = want["max_corners"], want["min_features"]
            n_old = [len(l.tracks) for l in loops]
            if want["land"] is not None:
                l0 = loops[0]
                seen = len(logs[0])
                _, st = track(l0.lk, l0.g_prev, io.gray_bgr8(frames[0, t]), l0.tracks)
                del logs[0][seen:]                              # the look ahead is no step
                mc = want["land"] + n_old[0] - int((st == 1).sum())
                mf = mc
            elif kind == "zero":
                mf = sorted(n_old[b] for b in range(B_STREAMS) if b != BLANK_STREAM)[1]
            step_cfg = dataclasses.replace(cfg, max_corners=mc)
            lks = [None] * B_STREAMS
            if variant == "seed":
                old = np.zeros((B_STREAMS, max_corners, 2), np.float32)
                for b in range(B_STREAMS):
                    old[b, :n_old[b]] = loops[b].tracks
                sd = seeds(old, np.array(n_old, np.int32), sens)
                lks = [(lambda g0, g1, o, s=sd[b, :n_old[b]]: R.lk_pyr(g0, g1, o, cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr,
                                                                       seed=s, flags=R.USE_INITIAL_FLOW)) for b in range(B_STREAMS)]
            row = []
            for b, l in enumerate(loops):
                l.cfg, l.min_feat = step_cfg, mf
                o = l.step(frames[b, t], sens[b], lk=lks[b])
                if variant == "gate":                            # the tracker is not asked without tracks: the gate's result is empty then
                    o["gate"] = logs[b][-1] if n_old[b] else G.gated(None, None, np.zeros((0, 2), np.float32), cfg.win, cfg.max_level, cfg.max_count,
                                                                     cfg.eps, cfg.min_eig_thr, None)
                row.append(o)
            steps.append(row); asked.append((mc, mf))
        return dict(first=first, steps=steps, asked=asked, cfg=cfg, sensors=sens)
    if variant == "seed":                                        # depends on the device's predictor: not cached
        return make()
    return cached(("stream", kind, max_corners, min_features, radius, variant, drop), make)


def trajectory(run, b):
    """[(n_old, n_tracked, count after)] of stream b."""
    return [(o["n_old"], o["n_tracked"], len(o["tracks"])) for o in (row[b] for row in run["steps"])]


# the replace re-detection (of_module.py:83-86): the script's loop in pixels, the LK flow, a threshold that keeps most points
MODULE_MIN_FEATURES = 590


def module_cfg(max_corners=600):
    from of_amd import ofk
    cfg = stream_cfg(max_corners)
    cfg.solve_variant = ofk.SOLVE_OFMODULE; cfg.feas_T = -0.5
    return cfg


def module_run(kind):
    """stream_oracle.oracle_of_module per stream -> dict(refs [b] = (first, steps), controls, omegas [NF-1,B,3], cx, cy, normal)."""
    def make():
        from of_amd.of_library import pix_trans
        frames, _ = stream_frames(kind == "zero")
        rng = np.random.default_rng(77)
        controls = rng.normal(0, 0.01, (NF - 1, B_STREAMS, 3)); omegas = rng.normal(0, 0.01, (NF - 1, B_STREAMS, 3))
        cx, cy = pix_trans((H, W))
        normal = np.array([0.0, 0.0, 1.0])
        from of_amd.pipeline import FusionConfig
        model = FusionConfig.of_module(synthetic_flow=False).model
        refs = [oracle_of_module(frames[b], module_cfg(), normal, controls[:, b], omegas[:, b], MODULE_MIN_FEATURES, cx, cy, model, False)
                for b in range(B_STREAMS)]
        return dict(refs=refs, controls=controls, omegas=omegas, cx=cx, cy=cy, normal=normal)
    return cached(("module", kind), make)


# ------------------------------------------------------------------------------------------------ section 2e: the pair chain
PAIR_CORNERS = 600
PAIR_SEEDS = rr.SCENE_SEEDS[:4]
PAIR_OBJECT = dict(size=(80, 110), at=(30, 40), step=(3, -4))  # robust_reference.scene at half size: rows, columns
PAIR_SETTING = dict(loss="tukey", c=4.685, iters=5, hypotheses=64, seed=0x1234ABCD5678)


def pair_cfg():
    from of_amd.pipeline import PipelineConfig
    return PipelineConfig(max_corners=PAIR_CORNERS, quality=0.001, min_distance=5, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)


def pair_scenes():
    """The moving-object scene of robust_reference.scene at 240 x 320 for four seeds: a textured rectangle of 80 x 110 pasted at
    (30, 40) in prev and (33, 36) in next.  -> (info of the first pair, prev [4,h,w,3], next [4,h,w,3])."""
    def make():
        s = synth()
        oh, ow = PAIR_OBJECT["size"]; r, c = PAIR_OBJECT["at"]; dr, dc = PAIR_OBJECT["step"]
        prev, nxt, info = [], [], None
        for seed in PAIR_SEEDS:
            pair = s.render_pair(H, W, seed, margin=96, **rr.TRUTH)
            a, b = pair["prev"].copy(), pair["next"].copy()
            tex = s.render_pair(oh + 40, ow + 40, seed + 100, margin=96)["prev"][20:20 + oh, 20:20 + ow]
            a[r:r + oh, c:c + ow] = tex; b[r + dr:r + dr + oh, c + dc:c + dc + ow] = tex
            prev.append(a); nxt.append(b); info = info or pair
        return info, np.stack(prev), np.stack(nxt)
    return cached("pairs", make)


def pair_problem(out, b, sr):
    """x, u, valid of pair b from downloaded (or oracle) points, as the device's solve forms them."""
    n = int(out["counts"][b])
    new = out["next_pts"][b, :n].astype(np.float64); old = out["prev_pts"][b, :n].astype(np.float64)
    return (new - [sr[20], sr[21]]) * sr[19], (new - old) * sr[19], out["status"][b, :n] == 1
