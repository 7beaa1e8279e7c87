"""CPU: the cases of tests/point_count_cases.py are not vacuous.  Every reference case of tests/test_gpu_point_counts.py and
tests/test_gpu_stream_counts.py runs here, and what makes the device comparison mean something is asserted on the reference alone:
every chunk of 256 points holds tracked, lost, far and capped points; the stream plans go past 512 (256) tracks, cross the boundary,
land on it and one above it, fill the re-detection budget, lose every track and refill; the robust solve rejects and keeps points
of index >= 512 under the conditions of tests/test_gpu_robust.py; the gate removes points of index >= 256.
A case that fails here gets other inputs; the limits stay."""
import numpy as np
import pytest

from oracle import image_oracle as io
import lk_seed_reference as R  # noqa: E402  (tests/lk_seed_reference.py)
import track_gate_reference as G  # noqa: E402  (tests/track_gate_reference.py)
import robust_reference as rr  # noqa: E402  (tests/robust_reference.py)
import point_count_cases as P  # noqa: E402  (tests/point_count_cases.py)
from point_count_cases import bits


def test_point_set_and_counts(pkg):
    p = P.points()
    assert p.shape == (P.S, 2) and p.dtype == np.float32
    outside = (p[:, 0] < 0) | (p[:, 0] > P.W - 1) | (p[:, 1] < 0) | (p[:, 1] > P.H - 1)
    for lo, hi in ((0, 256),) + P.CHUNKS:
        assert outside[lo:hi].sum() >= 3, (lo, int(outside[lo:hi].sum()))        # border and outside points in every chunk
    assert {c % 4 for c in P.COUNTS} == {0, 1, 2, 3} and {0, 1, 255, 256, 257, 511, 512, 513, 768, 769, 1024, P.S} <= set(P.COUNTS)
    assert all(len(g) == 4 for g in P.GROUPS) and sum(P.GROUPS, ()) == P.COUNTS


@pytest.mark.parametrize("case", P.GATE_CASES, ids=P.gate_id)
def test_every_chunk_of_the_gate_cases_is_busy(pkg, case):
    """Per chunk 1, 2, 3: at least 20 forward-tracked, 1 lost in the backward pass, 20 far; with the cap at least 5 capped, 20 kept."""
    win, var, fseed, cap = case
    c = P.gate_case(*case)
    r, gate = c["ref"], c["gate"]
    lost, far, capped, keep = P.gate_masks(r, gate)
    assert np.array_equal(r["stats"], [(r["st_f"] == 1).sum(), lost.sum(), far.sum(), capped.sum()])      # the masks are the reference's counts
    for lo, hi in P.CHUNKS:
        fig = (int((r["st_f"][lo:hi] == 1).sum()), int(lost[lo:hi].sum()), int(far[lo:hi].sum()), int(capped[lo:hi].sum()), int(keep[lo:hi].sum()))
        print(f"{P.gate_id(case)} points {lo}-{hi - 1}: tracked {fig[0]} lost {fig[1]} far {fig[2]} capped {fig[3]} kept {fig[4]}")
        assert fig[0] >= 20 and fig[1] >= 1 and fig[2] >= 20, (lo, fig)
        if cap:
            assert fig[3] >= 5 and fig[4] >= 20, (lo, fig)
    if fseed:
        plain = P.gate_case(win, var)["ref"]
        assert not np.array_equal(bits(plain["next"]), bits(r["next"]))            # the forward seed changes the outcome


def test_prefix_is_the_reference_of_fewer_points(pkg):
    """The device tests cut the reference of 1030 points to each count; a direct call gives the same."""
    s = P.scene()
    for case, counts in (((15, "plain-L2", False, True), (257, 7)), ((21, "plain-L2", True, False), (513,)), ((5, "seeded-L0", False, False), (64,))):
        win, var, fseed, cap = case
        c = P.gate_case(*case)
        for n in counts:
            want = G.gated(s["g0"], s["g1"], P.points()[:n], win, gate=c["gate"], seed=None if c["seed"] is None else c["seed"][:n], flags=c["flags"], **P.LK)
            got = P.prefix(c["ref"], c["gate"], n)
            for k in ("next", "status", "st_f", "err", "back", "st_b", "fb2", "stats"):
                assert np.array_equal(bits(got[k]), bits(want[k])), (case, n, k)
    assert not P.prefix(P.gate_case(15, "plain-L2")["ref"], P.gate_case(15, "plain-L2")["gate"], 0)["stats"].any()


def test_threshold_edges_exist(pkg):
    edges = P.threshold_edges()
    assert len(edges) == 3 and [i // 256 for i, *_ in edges] == [0, 1, 2], edges
    for i, d, thr_keep, thr_far in edges:
        below = np.nextafter(d, np.float32(-np.inf), dtype=np.float32)
        assert np.float32(thr_keep * thr_keep) == d and np.float32(thr_far * thr_far) == below and below < d
        a, b = P.gate_case(15, "plain-L2", fb_thr=thr_keep), P.gate_case(15, "plain-L2", fb_thr=thr_far)
        ka, kb = P.gate_masks(a["ref"], a["gate"]), P.gate_masks(b["ref"], b["gate"])
        assert ka[3][i] and not ka[1][i] and kb[1][i] and not kb[3][i], (i, d)
        print(f"point {i}: fb2 {d!r} kept at fb_thr {thr_keep!r} ({int(ka[3].sum())} kept, {int(ka[1].sum())} far), far at {thr_far!r}")
        assert ka[3].sum() >= 20 and ka[1].sum() >= 20                               # both outcomes on either side of the edge


@pytest.mark.parametrize("flags,L", P.LK_FLAG_CASES, ids=[f"flags{f}-L{L}" for f, L in P.LK_FLAG_CASES])
def test_flagged_lk_cases(pkg, flags, L):
    """The gate cases' limits for tracked and lost points, per chunk."""
    nxt, st, err = P.lk_case(flags, L)
    for lo, hi in P.CHUNKS:
        tracked, lost = int(st[lo:hi].sum()), int((st[lo:hi] == 0).sum())
        print(f"flags {flags} L {L} points {lo}-{hi - 1}: tracked {tracked} lost {lost}")
        assert tracked >= 20 and lost >= 1, (lo, tracked, lost)
    s = P.scene()
    seed = P.forward_seed() if flags & R.USE_INITIAL_FLOW else None
    n, sts, e = R.lk_pyr(s["g0"], s["g1"], P.points()[:258], 15, L, seed=None if seed is None else seed[:258], flags=flags, **P.LK_PARAMS)
    assert np.array_equal(bits(n.reshape(-1, 2)), bits(nxt[:258])) and np.array_equal(sts.ravel(), st[:258]) and np.array_equal(bits(e.ravel()), bits(err[:258]))
    if flags & R.GET_MIN_EIGENVALS:
        assert not np.array_equal(bits(err), bits(P.lk_case(flags & ~R.GET_MIN_EIGENVALS, L)[2] if flags & R.USE_INITIAL_FLOW else
                                                  R.lk_pyr(s["g0"], s["g1"], P.points(), 15, L, **P.LK_PARAMS)[2].ravel()))


def show(run, name):
    print(f"{name}: asked (max_corners, min_features) per step {run['asked']}")
    for b in range(P.B_STREAMS):
        print(f"    stream {b}: begin {len(run['first'][b])}, (n_old, n_tracked, after) {P.trajectory(run, b)}")


@pytest.mark.parametrize("max_corners,min_features", list(P.RUNS), ids=[f"{a}-{b}" for a, b in P.RUNS])
def test_stream_plans_reach_the_chunk_edges(pkg, max_corners, min_features):
    """The runs of point_count_cases.LANDING land on their boundary and one above it; (600, 590) re-detects in every step."""
    run = P.stream_run("edges", max_corners, min_features)
    show(run, f"edges {max_corners}-{min_features}")
    edge = 512 if max_corners > 512 else 256
    steps = [(o, mc) for row, (mc, _) in zip(run["steps"], run["asked"]) for o in row]
    assert any(o["n_old"] > edge for o, _ in steps)
    assert any(len(o["tracks"]) - o["n_tracked"] == mc - o["n_old"] > 0 for o, mc in steps)        # a re-detection cut by its budget
    if (max_corners, min_features) in P.LANDING:
        t0 = P.trajectory(run, 0)
        assert any(tr < edge <= after for _, tr, after in t0)
        assert t0[-2][2] == edge and t0[-1][0] == edge and t0[-1][2] == edge + 1, t0                # lands on 512, runs at 512, lands on 513
    else:
        assert all(o["n_tracked"] >= 512 for o, _ in steps) and sum(len(o["tracks"]) > o["n_tracked"] for o, _ in steps) >= 12
    lost_late = sum(int(o["n_old"] - o["n_tracked"]) for o, _ in steps)
    assert lost_late >= 20                                                                        # the compaction has gaps to close


def test_stream_plan_reaches_zero_tracks(pkg):
    run = P.stream_run("zero", 600, 590)
    show(run, "zero")
    t1 = P.trajectory(run, P.BLANK_STREAM)
    assert any(n_old > 0 and tr == 0 and after == 0 for n_old, tr, after in t1)                   # all tracks lost
    assert any(n_old == 0 and after == 0 for n_old, tr, after in t1)                              # nothing to re-detect on a blank frame
    assert any(n_old == 0 and after == 600 for n_old, tr, after in t1)                            # the refill
    assert not any(o["solved"] for o in (row[P.BLANK_STREAM] for row in run["steps"]) if o["n_tracked"] == 0)
    for t, (row, (mc, mf)) in enumerate(zip(run["steps"], run["asked"])):
        if row[P.BLANK_STREAM]["n_old"] == 0:                    # budgets of 0 (no re-detection), a few and max_corners in one call
            others = [o["n_old"] for b, o in enumerate(row) if b != P.BLANK_STREAM]
            assert any(n > mf for n in others) and any(0 < mc - n < 100 and n <= mf for n in others), (t, others, mf)


def test_stream_plans_of_the_mask_radius(pkg):
    for mc, mf, radius in ((600, 590, 0), (300, 256, 0), (600, 590, 255)):
        run = P.stream_run("edges", mc, mf, radius=radius)
        show(run, f"edges {mc}-{mf} radius {radius}")
        steps = [o for row in run["steps"] for o in row]
        if radius == 255:
            assert all(len(o["tracks"]) == o["n_tracked"] for o in steps) and sum(o["n_old"] <= mf for o in steps) >= 8
        else:
            assert any(len(o["tracks"]) > o["n_tracked"] for o in steps)
    a, b = P.stream_run("edges", 600, 590, radius=0), P.stream_run("edges", 600, 590)
    assert any(not np.array_equal(x["tracks"], y["tracks"]) for ra, rb in zip(a["steps"], b["steps"]) for x, y in zip(ra, rb))   # the radius matters


@pytest.mark.parametrize("kind", ["edges", "zero"])
@pytest.mark.parametrize("variant,drop", [("kf3", False), ("gate", False), ("robust", False), ("robust-fused", True), ("seed", False)],
                         ids=["kf3", "gate-seeded-L0", "robust-step-keep", "robust-fused-drop", "lk-seed-model"])
def test_stream_variant_plans(pkg, kind, variant, drop):
    seeds = None
    if variant == "seed":                                        # the device test takes the device's predictor (at most one ulp from this one)
        seeds = lambda old, counts, sens: np.stack([R.predict(old[b], sens[b], R.SEED_MODEL, 1.0) for b in range(len(old))])
    run = P.stream_run(kind, 600, 590, variant=variant, drop=drop, seeds=seeds)
    show(run, f"{kind} {variant} drop {drop}")
    steps = [o for row in run["steps"] for o in row]
    assert any(o["n_old"] > 512 for o in steps)
    if kind == "zero":
        assert any(o["n_old"] == 0 for o in steps) and any(o["n_old"] == 0 and len(o["tracks"]) == 600 for o in steps)
    if variant in ("robust", "robust-fused"):
        for o in steps:
            assert o["gap"] >= 1e-6 and o["near"] == 0, (o["gap"], o["near"])
        late = [(int(np.count_nonzero((o["weights"][512:] == 0) & o["valid"][512:])), int(np.count_nonzero(o["weights"][512:] > 0))) for o in steps]
        print("    tracked points of index >= 512 at weight 0 / above 0, per step and stream:", late)
        assert any(z >= 5 and p >= 5 for z, p in late)
        if drop:
            assert any(o["keep"].sum() < o["n_tracked"] for o in steps)            # and with drop they leave the tracks
    if variant == "gate":
        gate = dict(fb="seeded", fb_thr=0.5)
        pruned = 0
        for o in steps:
            lost, far, _, _ = P.gate_masks(o["gate"], gate)
            pruned += int(lost[256:].sum() + far[256:].sum())
        print("    points of index >= 256 the gate removed:", pruned)
        assert pruned >= 5
    if variant == "seed":
        plain = P.stream_run(kind, 600, 590)
        assert any(not np.array_equal(x["tracks"], y["tracks"]) for ra, rb in zip(run["steps"], plain["steps"]) for x, y in zip(ra, rb))


@pytest.mark.parametrize("kind", ["edges", "zero"])
def test_replace_plan(pkg, kind):
    m = P.module_run(kind)
    for b, (first, steps) in enumerate(m["refs"]):
        print(f"replace {kind} stream {b}: begin {len(first)}, (n_old, n_kept, solved) {[(s[4], s[5], s[0] is not None) for s in steps]}")
    steps = [s for _, st in m["refs"] for s in st]
    assert any(s[4] > 512 for s in steps) and any(256 < s[4] <= 512 for s in steps) and any(s[4] < 64 for s in steps)
    assert sum(s[4] != P.PAIR_CORNERS and s[4] > 0 for s in steps) >= 8                          # replaced again and again
    if kind == "zero":
        z = m["refs"][P.BLANK_STREAM][1]
        assert any(s[4] == 0 and s[0] is None for s in z) and any(s[4] == 600 for s in z[3:])


def test_pair_scenes_hold_600_corners_and_meet_the_robust_conditions(pkg):
    info, prev, nxt = P.pair_scenes()
    cfg = P.pair_cfg()
    sr = P.sensor_rows(info, 1)[0]
    kw = dict(P.PAIR_SETTING, loss=rr.TUKEY)
    for i in range(len(prev)):
        g0, g1 = io.gray_bgr8(prev[i]), io.gray_bgr8(nxt[i])
        pts = io.good_features(g0, cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size)
        assert len(pts) == P.PAIR_CORNERS
        n, s, e = io.lk_pyr(g0, g1, pts, cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr)
        out = dict(counts=[len(pts)], next_pts=n.reshape(1, -1, 2), prev_pts=pts.reshape(1, -1, 2), status=s.reshape(1, -1))
        x, u, ok = P.pair_problem(out, 0, sr)
        for problem in range(i, 128, len(prev)):                 # the batch of 128 repeats the scenes: another sample per pair
            r = rr.robust_solve(rr.NODE, x, u, sr[0], sr[1:4], sr[4:7], valid=ok, problem=problem, **kw)
            assert r["gap"] >= 1e-6 and r["near"] == 0 and r["stats"][7] == 0, (i, problem, r["gap"], r["near"], r["stats"])
            zero, kept = int(np.count_nonzero((r["weights"][512:] == 0) & ok[512:])), int(np.count_nonzero(r["weights"][512:] > 0))
            assert zero >= 5 and kept >= 5, (i, problem, zero, kept)
        plain = rr.robust_solve(rr.NODE, x, u, sr[0], sr[1:4], sr[4:7], valid=ok, problem=i, **dict(kw, iters=0, hypotheses=0))
        print(f"pair scene {i}: {len(pts)} corners, {int(ok.sum())} tracked, of index >= 512: {zero} at weight 0, {kept} above; "
              f"error plain {rr.rel_err(plain['v'], info['v']):.3f} robust {rr.rel_err(r['v'], info['v']):.4f}")
        assert rr.rel_err(plain["v"], info["v"]) >= rr.PLAIN_MIN and rr.rel_err(r["v"], info["v"]) <= rr.ROBUST_MAX
