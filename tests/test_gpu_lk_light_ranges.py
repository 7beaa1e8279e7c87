"""GPU parity of the lighting-insensitive LK (k_lk_light<15|21|31, FLAGS>, csrc/k_lk_light.inc, launched by ofk_launch_lk_light)
over its whole window and parameter range, against tests/lk_light_reference.py: `next` and `err` as uint32 and `status` exactly,
per image over its own count, in both modes, no tolerance anywhere.  The inputs are built by tests/lk_light_ranges.py;
tests/test_lk_light_ranges_reference.py shows from the reference alone that each of them keeps the tracker live.

 1. every window     odd 3..31 on a dword-width and an odd-width frame, plain and seeded 12 px off with the eigenvalue flag, and
                     seeded on level 0 alone, where the staged next-frame region is left; the routing thresholds at 15 and 21
                     restated, all three kernels seen
 2. full contrast    binary noise, plaid and a half-stripes frame against rolled copies at full and quarter brightness: the 32-bit
                     DPP row sums of windows <= 15 past 2^31 (restated in numpy and printed), the 64-bit sums of <21> and <31>
 3. constant frames  next frames all 255 / 0 / 100: vJ = 0 at every step, full rows of 64 * 8160^2, a drift across restagings;
                     the three give the same bits
 4. gain_max range   1.0000001 .. 1e300 on a pair sixteen times apart in gain, either way round: both bounds of the clamp bind
 5. termination      the max_count x eps x min_eig grid, the launcher's clamps, max_count 0 (rule 6 at the start position)
 6. level cuts       pyramids cut one and two halvings down at max_level 8, on a context of nine levels
 7. gates            ofk_lk_pyr_fb under the light: fb plain / seeded, fb_level -1 / 0 / 1, err_max off / on, a ragged batch
 8. far coordinates  a point and seeds at +-1e6 among ordinary points
"""
import numpy as np
import pytest

import lk_light_ranges as lr
import lk_seed_reference as R  # noqa: E402  (tests/lk_seed_reference.py)
from oracle import image_oracle as io
from test_gpu_lk_seed import bits
from test_gpu_lk_light import check

pytestmark = pytest.mark.gpu


def on_device(ctx, case, light):
    """The case through ofk_lk_pyr_light, held to the reference (test_gpu_lk_light.check) -> (next [B,S,2], status [B,S], err [B,S])."""
    return check(ctx, case.g0, case.g1, case.pts, case.counts, case.win, case.L, case.seed, case.flags, light, case.tag, case.lk)


def same_bits(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------- 1. every window
def test_light_every_window(gpu_ctx, pkg):
    seen, frac, restaged = set(), {}, {}
    for case in lr.every_window_cases():
        seen.add(lr.light_kernel(case.win))
        for mode in lr.MODES:
            nxt, st, _ = on_device(gpu_ctx, case, mode)
            if case.flags == 0:
                frac.setdefault((case.win, mode), []).append(st[0, -case.inner:])
            if case.L == 0:
                restaged[case.win, mode] = restaged.get((case.win, mode), 0) + int(lr.restaged_rows(case, nxt[0], st[0]).sum())
    frac = {k: float(np.concatenate(v).mean()) for k, v in frac.items()}
    assert min(frac.values()) >= 0.6, frac                       # tracked: the comparison is not one of lost points
    assert min(restaged.values()) >= 1, restaged                 # the next-frame region was restaged behind a tracked point
    assert seen == lr.LIGHT_KERNELS, seen
    assert [lr.light_kernel(w) for w in (15, 17, 21, 23)] == ["k_lk_light<15>", "k_lk_light<21>", "k_lk_light<21>", "k_lk_light<31>"]
    print("k_lk_light<15>, k_lk_light<21> and k_lk_light<31> all ran: windows " +
          "; ".join(f"{k} {[w for w in lr.WINDOWS if lr.light_kernel(w) == k]}" for k in sorted(seen)))


# ---------------------------------------------------------------------------------------------------- 2. full contrast
def test_light_full_contrast_every_kernel(gpu_ctx, pkg):
    """The sums of the integer-position points at their start position are restated in numpy (lk_light_ranges.row_sums): the jv^2 row
    sum passes 2^31 at window 15, so only its unsigned reading is right."""
    imgs, ipts, _ = lr.full_contrast_inputs()
    seen, peak = set(), {}
    for case in lr.full_contrast_cases():
        seen.add(lr.light_kernel(case.win))
        for mode in lr.MODES:
            on_device(gpu_ctx, case, mode)
        if case.win <= 15:
            top = np.max([lr.row_sums(case.g0[b], case.g1[b], ipts, case.win) for b in range(3)], axis=0)
            peak[case.win] = np.maximum(peak.get(case.win, 0), top)
    assert seen == lr.LIGHT_KERNELS, seen
    for win, top in sorted(peak.items()):
        print(f"window {win:2d}: peak 32-bit row sum of jv^2 {int(top[0])} ({top[0] / 2 ** 32:.3f} of 2^32), of |jv ix| {int(top[1])} "
              f"({top[1] / 2 ** 31:.3f} of 2^31), of |jv iy| {int(top[2])} ({top[2] / 2 ** 31:.3f} of 2^31)")
    assert peak[15][0] > 2 ** 31, peak
    assert all(t[0] < 2 ** 32 and max(t[1], t[2]) < 2 ** 31 for t in peak.values()), peak


# ---------------------------------------------------------------------------------------------------- 3. constant next frames
def test_light_constant_next_frames(gpu_ctx, pkg):
    """In gain mode every step takes the vJ <= 0 branch; N SJx - SJ SIx and N pJ - SJ vanish identically, so the mismatch vector is
    the template's half, the point drifts for all max_count steps, and 255, 0 and 100 give the same bits in both modes."""
    for case in lr.constant_cases():
        for mode in lr.MODES:
            got = on_device(gpu_ctx, case, mode)
            for b in (1, 2):
                assert same_bits([g[0] for g in got], [g[b] for g in got]), (case.tag, mode, lr.CONST_VALUES[b])
            assert got[1][0].sum() >= 48, (case.tag, mode)


# ---------------------------------------------------------------------------------------------------- 4. clamp and gain_max range
def test_light_gain_max_range(gpu_ctx, ofk, pkg):
    for case in lr.clamp_cases():
        got = [on_device(gpu_ctx, case, ofk.lk_light_setting("gain", g)) for g in lr.GAIN_MAX]
        for g, a, b in zip(lr.GAIN_MAX[1:-1], got, got[1:-1]):    # consecutive values up to 1e3 differ
            assert np.any(bits(a[0]) != bits(b[0])), (case.tag, g)
        assert same_bits(got[-2], got[-1]), case.tag               # 1e3 and 1e300: the clamp no longer binds
        lo = on_device(gpu_ctx, case, ofk.lk_light_setting("bias", 1.5))
        hi = on_device(gpu_ctx, case, ofk.lk_light_setting("bias", 1e300))
        assert same_bits(lo, hi), case.tag                         # bias mode does not read gain_max
        assert np.any(bits(lo[0]) != bits(got[-1][0])), case.tag


# ---------------------------------------------------------------------------------------------------- 5. termination grid
def test_light_termination_criteria_and_clamps(gpu_ctx, pkg):
    seen = set()
    for base, combos in lr.criteria_cases():
        seen.add(lr.light_kernel(base.win))
        n = base.inner
        for mode in lr.MODES:
            res = {c: on_device(gpu_ctx, lr.with_criteria(base, *c), mode) for c in combos}
            for mc, eps, thr in combos:                           # the launcher's clamps: 150 runs as 100, eps 20 as 10
                for a, b in (((150, eps, thr), (100, eps, thr)), ((mc, 20.0, thr), (mc, 10.0, thr))):
                    if a in res and b in res:
                        assert same_bits(res[a], res[b]), (base.tag, mode, a, b)
            # max_count 0: the loop is skipped, rule 6 runs at the start position
            nxt, st, err = res[next(c for c in combos if c[0] == 0 and c[2] <= 1e-4)]
            assert st[0, :n].all() and np.array_equal(bits(nxt[0, :n]), bits(base.pts[0, :n])) and (err[0, :n] > 0).all(), (base.tag, mode)
            nxt, st, err = on_device(gpu_ctx, lr.with_criteria(base, 0, 0.03, 1e-4, R.USE_INITIAL_FLOW), mode)
            assert st[0].sum() >= n and np.array_equal(bits(nxt[0][st[0] == 1]), bits(base.seed[0][st[0] == 1])), (base.tag, mode)
            for mc in (1, 2):                                     # seeded, a step or two: never the oscillation rule / once
                on_device(gpu_ctx, lr.with_criteria(base, mc, 0.0, 1e-4, lr.SEED_EIG), mode)
    assert seen == lr.LIGHT_KERNELS, seen


# ---------------------------------------------------------------------------------------------------- 6. level cuts
@pytest.fixture(scope="module")
def ctx9(ofk):
    """A small context of its own with all nine pyramid levels."""
    c = ofk.Context(0, 320, 256, 16, 256, 8)
    yield c
    c.close()


def test_light_level_cut(ctx9, pkg):
    """Frames whose (n + 1) / 2 chain lands on win (cut) or win + 1 (kept) one or two halvings down, at max_level 8."""
    for win in (3, 15, 31):
        depths = set()
        for case in lr.level_cut_cases((win,)):
            assert io.lk_levels(*case.geom, win, 8) == case.depth, case.tag
            depths.add(case.depth)
            for mode in lr.MODES:
                on_device(ctx9, case, mode)
        assert len(depths) >= 2, (win, depths)


# ---------------------------------------------------------------------------------------------------- 7. gates under the light
@pytest.mark.parametrize("win", lr.GATE_WINDOWS)
def test_light_gates(gpu_ctx, pkg, win):
    """ofk_lk_pyr_fb with the light on against lk_light_reference.gated, all six outputs; per setting the gate it is about fires in
    the reference (the forward-backward check; with err_max on the cap, which reads rule 6's err)."""
    g0, g1, pts, counts = scene = lr.gate_scene(pkg, win)
    for gate in lr.gate_settings():
        for mode in lr.MODES:
            out = gpu_ctx.lk_pyr_fb(g0, g1, pts, counts, win=win, max_level=3, light=mode, **gate, **lr.LK)
            ref = lr.gated_reference(scene, win, 3, gate, mode)
            for b, (c, r) in enumerate(zip(counts, ref)):
                for k, rk in (("next_pts", "next"), ("status", "status"), ("err", "err"), ("back_pts", "back"), ("back_status", "st_b"), ("fb2", "fb2")):
                    assert np.array_equal(bits(out[k][b, :c]), bits(r[rk])), (win, mode, gate, "image", b, k)
            stats = np.sum([r["stats"] for r in ref], axis=0)
            assert stats[1] + stats[2] >= 1, (win, mode, gate, stats)
            assert gate["err_max"] == 0.0 or stats[3] >= 1, (win, mode, gate, stats)


# ---------------------------------------------------------------------------------------------------- 8. far coordinates
def test_light_far_coordinates(gpu_ctx, pkg):
    """A point at (-1e6, 3) and seeds of (1e6, -1e6) and (999999.5, 20): inside int, out of bounds at every level -> status 0, the
    reference's `next` bits, and the other points as in the call without them."""
    rows = [lr.FAR_POINT, *lr.FAR_SEEDS]
    for far, near in lr.far_cases():
        for mode in lr.MODES:
            f, n = on_device(gpu_ctx, far, mode), on_device(gpu_ctx, near, mode)
            assert not f[1][0, rows].any() and n[1][0, rows].all(), (far.tag, mode)
            rest = np.setdiff1d(np.arange(f[1].shape[1]), rows)
            assert same_bits([a[0, rest] for a in f], [a[0, rest] for a in n]), (far.tag, mode)
