"""GPU: the stage entries of the tracking chain over point counts from 0 to 1030 per image (tests/point_count_cases.py: COUNTS), so
that every kernel's second and third pass of 256 threads, its partly filled last pass, its sums over the four waves and the four
residues of k_lk15q's points-per-wave packing are compared, not only its first wave.

(a) ofk_lk_pyr_fb against tests/track_gate_reference.py over windows 5 (k_lk15), 15 (k_lk15q) and 21 (k_lk_f<21>), plain and seeded
    backward passes, the err cap and a seeded forward pass: six point arrays bit for bit, the four counts exactly, from the call and
    from ofk_track_gate_download.
(b) the gate's threshold at the edge of one float32: fb_thr values whose rounded square is a kept point's distance, and the float32
    just below it, for a point of each of the first three chunks.
(c) ofk_lk_pyr_ex under the cv2 flags and ofk_predict_points over the same counts; what lies beyond an image's count stays as it was.
tests/test_point_count_cases.py asserts on the reference alone that every chunk of these inputs holds tracked, lost, far and capped
points: a comparison in which nothing happens beyond the first 256 points proves nothing."""
import numpy as np
import pytest

import lk_seed_reference as R  # noqa: E402  (tests/lk_seed_reference.py)
import point_count_cases as P  # noqa: E402  (tests/point_count_cases.py)
from point_count_cases import bits

pytestmark = pytest.mark.gpu


def batch_of(group, arr, tail=None):
    """[4,S,...]: every image gets the same S entries; with `tail`, those at or beyond its count are set to it."""
    out = np.repeat(np.asarray(arr)[None], len(group), 0).copy()
    if tail is not None:
        for b, c in enumerate(group):
            out[b, c:] = tail
    return out


def frames(group):
    s = P.scene()
    return np.repeat(s["g0"][None], len(group), 0), np.repeat(s["g1"][None], len(group), 0)


def assert_gate_group(ctx, group, case, win, tag):
    gate, ref = case["gate"], case["ref"]
    prev, nxt = frames(group)
    counts = np.array(group, np.int32)
    seed = None if case["seed"] is None else batch_of(group, case["seed"])
    out = ctx.lk_pyr_fb(prev, nxt, batch_of(group, P.points()), counts, win=win, next_pts=seed, flags=case["flags"], **gate, **P.LK)
    dl = ctx.track_gate_download(len(group))
    for b, c in enumerate(group):
        r = P.prefix(ref, gate, c); t = (tag, "count", c)
        for name, key in (("next_pts", "next"), ("status", "status"), ("err", "err"), ("back_pts", "back"), ("back_status", "st_b"), ("fb2", "fb2")):
            bad = P.differing(out[name][b, :c], r[key])
            assert bad.size == 0, (t, name, "first differing index", int(bad[0]), "chunk", int(bad[0]) // 256, "of", bad.size)
        assert np.array_equal(dl["stats"][b], r["stats"]), (t, "stats", dl["stats"][b], r["stats"])
        assert np.array_equal(bits(dl["fb2"][b, :c]), bits(r["fb2"])) and np.array_equal(bits(dl["back_pts"][b, :c]), bits(r["back"])), t
        assert np.array_equal(dl["back_status"][b, :c], r["st_b"]), t
    return out, dl


@pytest.mark.parametrize("case", P.GATE_CASES, ids=P.gate_id)
def test_gate_stage_entry_over_counts(pkg, gpu_ctx, case):
    win, var, fseed, cap = case
    c = P.gate_case(*case)
    for group in P.GROUPS:
        assert_gate_group(gpu_ctx, group, c, win, P.gate_id(case))


def test_gate_threshold_edge_in_three_chunks(pkg, gpu_ctx):
    """ofk.h: fb_thr is squared in double and rounded once to float32; a point whose float32 distance equals that value stays, one
    float32 below it the point is far."""
    edges = P.threshold_edges()
    assert len(edges) == 3 and [i // 256 for i, *_ in edges] == [0, 1, 2], edges
    group = (P.S, 769, 513, 257)                                 # the point of chunk 2 lies in the first two images only
    for i, d, thr_keep, thr_far in edges:
        for thr, kept in ((thr_keep, True), (thr_far, False)):
            c = P.gate_case(15, "plain-L2", fb_thr=thr)
            lost, far, capped, keep = P.gate_masks(c["ref"], c["gate"])
            assert bool(keep[i]) == kept and bool(far[i]) == (not kept) and c["ref"]["fb2"][i] == d, (i, d, thr, kept)
            out, dl = assert_gate_group(gpu_ctx, group, c, 15, ("edge", i, thr))
            for b, n in enumerate(group):
                if i < n:
                    assert out["status"][b, i] == (1 if kept else 0) and bits(out["fb2"][b, i:i + 1])[0] == bits(np.array([d], np.float32))[0], (i, thr, b)


@pytest.mark.parametrize("flags,L", P.LK_FLAG_CASES, ids=[f"flags{f}-L{L}" for f, L in P.LK_FLAG_CASES])
def test_flagged_lk_over_counts(pkg, ofk, gpu_ctx, flags, L):
    """USE_INITIAL_FLOW, GET_MIN_EIGENVALS and both (k_lk15q_f on level 0 and 1 of this size, k_lk15_f on level 2).  The start
    positions are LK's in/out array: beyond an image's count they carry a sentinel, which must come back."""
    want = P.lk_case(flags, L)
    seeded = bool(flags & R.USE_INITIAL_FLOW)
    for group in P.GROUPS:
        prev, nxt = frames(group)
        counts = np.array(group, np.int32)
        seed = batch_of(group, P.forward_seed(), tail=P.SENTINEL)
        got = gpu_ctx.lk_pyr(prev, nxt, batch_of(group, P.points()), counts, win=15, max_level=L, next_pts=seed if seeded else None, flags=flags, **P.LK_PARAMS)
        for b, c in enumerate(group):
            for name, g, r in zip(("next", "status", "err"), got, want):
                bad = P.differing(g[b, :c], r[:c])
                assert bad.size == 0, (flags, L, "count", c, name, "first differing index", int(bad[0]), "chunk", int(bad[0]) // 256, "of", bad.size)
            if seeded:
                assert np.all(bits(got[0][b, c:]) == bits(np.array([P.SENTINEL]))[0]), (flags, L, "count", c, "next_pts beyond the count were written")
        if seeded:
            # the same buffers, no start positions: the kernel must leave what lies beyond the counts where the seeded call left it
            plain = gpu_ctx.lk_pyr(prev, nxt, batch_of(group, P.points()), counts, win=15, max_level=L, flags=R.GET_MIN_EIGENVALS, **P.LK_PARAMS)
            for b, c in enumerate(group):
                assert np.all(bits(plain[0][b, c:]) == bits(np.array([P.SENTINEL]))[0]), (L, "count", c, "next_pts beyond the count were written")


def test_predict_points_over_counts(pkg, ofk, gpu_ctx):
    """k_seed_points: (stride + 255) / 256 blocks per image.  The rule of tests/test_gpu_lk_seed.py: at most one ulp from the numpy
    predictor; entries at or beyond an image's count come back as they went in (a sentinel here)."""
    total = differ = 0
    for group in P.GROUPS:
        counts = np.array(group, np.int32)
        sens = P.sensor_rows(P.scene()["pair"], len(group))
        sens[:, 22:25] *= np.arange(1, len(group) + 1)[:, None]  # another prior velocity per image
        pts = batch_of(group, P.points(), tail=P.SENTINEL)
        for mode in (ofk.SEED_MODEL, ofk.SEED_ROTATION):
            for gain in (1.0, 7.5):
                got = gpu_ctx.predict_points(pts, counts, sens, mode, gain)
                for b, c in enumerate(group):
                    want = R.predict(pts[b, :c], sens[b], mode, gain)
                    gi = got[b, :c].view(np.int32).astype(np.int64); wi = want.view(np.int32).astype(np.int64)
                    assert np.all(np.abs(gi - wi) <= 1), (mode, gain, "count", c, int(np.argmax(np.abs(gi - wi).max(1) > 1)))
                    assert np.any(gi != pts[b, :c].view(np.int32)) or c == 0, (mode, gain, c)       # the seeds are not the points
                    total += gi.size; differ += int(np.sum(gi != wi))
                    assert np.all(bits(got[b, c:]) == bits(np.array([P.SENTINEL]))[0]), (mode, gain, "count", c)
    print(f"ofk_predict_points over {len(P.COUNTS)} counts: {differ} of {total} values differ from the numpy predictor (each by one ulp)")
