"""CPU: every input of tests/test_gpu_lk_light_ranges.py (built by tests/lk_light_ranges.py) keeps the reference tracker
(tests/lk_light_reference.py) live - points are tracked, Newton steps are taken, the light changes the tracks, the gates reject - so
that a bit-for-bit comparison on those inputs is one of a working tracker and not of lost points.  No GPU and no statement about the
kernels: every figure is the reference's own, printed before it is held to its floor."""
import numpy as np
import pytest

import lk_light_ranges as lr
from test_gpu_lk_seed import bits

_differ = lambda a, b: int(np.sum(np.any(bits(a) != bits(b), axis=-1)))   # points whose (x, y) bits differ


# ---------------------------------------------------------------------------------------------------- 1. every window
def test_every_window_tracks_and_the_light_matters(pkg):
    """Corner points: status-1 share >= 0.6 at every window in both modes; >= 100 points per window whose `next` differs in bits from
    the same call with the light off."""
    share, differ, restaged = {}, {}, {}
    for case in lr.every_window_cases():
        off = case.reference(None)
        for mode in lr.MODES:
            nxt, st, _ = case.reference(mode)
            key = (case.win, mode, case.flags)
            share.setdefault(key, []).append(st[-case.inner:])
            differ[key] = differ.get(key, 0) + _differ(nxt, off[0])
            if case.L == 0:
                restaged[case.win, mode] = restaged.get((case.win, mode), 0) + int(lr.restaged_rows(case, nxt, st).sum())
    share = {k: float(np.concatenate(v).mean()) for k, v in share.items()}
    for win in lr.WINDOWS:
        print(f"window {win:2d}: corner share " + ", ".join(f"{m} {share[win, m, 0]:.3f} (seeded {share[win, m, lr.SEED_EIG]:.3f})" for m in lr.MODES) +
              "; next differs from light off at " + ", ".join(f"{m} {differ[win, m, 0]}" for m in lr.MODES) + " points; restaged on level 0 " +
              ", ".join(f"{m} {restaged[win, m]}" for m in lr.MODES))
    assert min(v for k, v in share.items() if k[2] == 0) >= 0.6, share
    assert min(v for k, v in differ.items() if k[2] == 0) >= 100, differ
    assert min(restaged.values()) >= 1, restaged                # every window restages behind a tracked point, in both modes
    assert {lr.light_kernel(w) for w in lr.WINDOWS} == lr.LIGHT_KERNELS


# ---------------------------------------------------------------------------------------------------- 2. full contrast
def test_full_contrast_frames_are_tracked(pkg):
    """Minimum over shifts, brightness and modes of the status-1 count out of 64: >= 32 on the noise and mixed frames at every odd
    window, on the plaid from window 11 up."""
    low = {}
    for case in lr.full_contrast_cases(lr.WINDOWS):
        for mode in lr.MODES:
            for b in range(3):
                n = int(case.reference(mode, b)[1].sum())
                low[case.name, case.win] = min(low.get((case.name, case.win), 64), n)
    for name in ("noise", "mixed", "plaid"):
        print(f"{name}: fewest tracked of 64, windows 3..31: " + ", ".join(str(low[name, w]) for w in lr.WINDOWS))
    assert all(low[name, w] >= 32 for name in ("noise", "mixed") for w in lr.WINDOWS), low
    assert all(low["plaid", w] >= 32 for w in lr.WINDOWS if w >= 11), low


def test_row_sums_pass_int32(pkg):
    """The restated 16-lane row sums: jv^2 passes 2^31 at window 15 (only the unsigned reading is right) and stays below 2^32, the
    signed products stay below 2^31."""
    imgs, ipts, _ = lr.full_contrast_inputs()
    for win in (w for w in lr.FULL_WINDOWS if w <= 15):
        top = np.max([lr.row_sums(img, np.roll(img, s, axis=(0, 1)) // div, ipts, win) for img in imgs.values() for s in lr.FULL_SHIFTS
                      for div in lr.FULL_DIVISORS], axis=0)
        print(f"window {win:2d}: peak row sum of jv^2 {int(top[0])} ({top[0] / 2 ** 32:.3f} of 2^32), of |jv ix| {int(top[1])} "
              f"({top[1] / 2 ** 31:.3f} of 2^31), of |jv iy| {int(top[2])}")
        assert top[0] < 2 ** 32 and max(top[1], top[2]) < 2 ** 31
        if win == 15:
            assert top[0] > 2 ** 31
    white = np.full((120, 160), 255, np.uint8)
    assert lr.row_sums(white, white, ipts, 15)[0] == 64 * 8160 ** 2


# ---------------------------------------------------------------------------------------------------- 3. constant next frames
def test_constant_next_frames_drift(pkg):
    """>= 48 of 64 points keep status 1 after all 20 steps, >= 16 moved by more than a pixel; 255, 0 and 100 give the same bits."""
    for case in lr.constant_cases():
        for mode in lr.MODES:
            res = [case.reference(mode, b, iters=True) for b in range(3)]
            nxt, st, err, it = res[0]
            moved = int(np.sum(np.linalg.norm(nxt - case.pts[0], axis=1)[st == 1] > 1.0))
            print(f"{case.tag} {mode}: {int(st.sum())} of 64 tracked, {moved} moved by more than a pixel, at most {int(it.max())} steps on a level")
            assert st.sum() >= 48 and moved >= 16, (case.tag, mode)
            assert it.max() == 20
            for other in res[1:]:
                assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(res[0][:3], other[:3])), (case.tag, mode)


# ---------------------------------------------------------------------------------------------------- 4. clamp and gain_max range
def test_gain_max_range_changes_the_tracks(pkg):
    """Consecutive gain_max values up to 1e3 give different tracks, 1e3 and 1e300 the same; bias mode does not read gain_max."""
    for case in lr.clamp_cases():
        res = [case.reference(("gain", g)) for g in lr.GAIN_MAX]
        d = [_differ(a[0], b[0]) for a, b in zip(res, res[1:])]
        print(f"{case.tag}: tracked {[int(r[1].sum()) for r in res]}; points that differ between consecutive gain_max {d}")
        assert min(d[:-1]) > 0 and d[-1] == 0, (case.tag, d)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(res[-2], res[-1]))
        assert int(res[-1][1].sum()) >= 48, case.tag            # tracked where the clamp does not bind; a tight clamp loses points
        lo, hi = case.reference(("bias", 1.5)), case.reference(("bias", 1e300))
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(lo, hi))
        assert _differ(lo[0], res[-1][0]) > 0                   # and the two modes are not one


# ---------------------------------------------------------------------------------------------------- 5. termination grid
def test_termination_grid_step_counts(pkg):
    """The largest Newton-step count on a level is 0, 1 and 2 at max_count 0, 1 and 2 and exceeds 2 at max_count 100, eps 0.03."""
    for base, combos in lr.criteria_cases():
        for mode in lr.MODES:
            most = {mc: int(lr.with_criteria(base, mc, 0.03, 1e-4).reference(mode, iters=True)[3].max()) for mc in (0, 1, 2, 100)}
            print(f"{base.tag} {mode}: most Newton steps on a level at max_count 0 / 1 / 2 / 100: {most[0]} / {most[1]} / {most[2]} / {most[100]}")
            assert (most[0], most[1], most[2]) == (0, 1, 2) and most[100] > 2, (base.tag, mode, most)
            n = base.inner                                      # max_count 0: every corner point keeps status 1, at its start position
            nxt, st, err = lr.with_criteria(base, 0, 0.03, 1e-4).reference(mode)
            assert st[:n].all() and np.array_equal(bits(nxt[:n]), bits(base.pts[0, :n])) and (err[:n] > 0).all()
            nxt, st, err = lr.with_criteria(base, 0, 0.03, 1e-4, lr.R.USE_INITIAL_FLOW).reference(mode)
            assert st[:n].all() and np.array_equal(bits(nxt[st == 1]), bits(base.seed[0][st == 1]))


# ---------------------------------------------------------------------------------------------------- 6. level cuts
def test_level_cut_frames_are_tracked(pkg):
    from oracle import image_oracle as io
    for win in (3, 15, 31):
        cases = list(lr.level_cut_cases((win,)))
        assert len({c.depth for c in cases}) >= 2
        for c in cases:
            assert io.lk_levels(*c.geom, win, 8) == c.depth
        tracked = {m: sum(int(c.reference(m)[1].sum()) for c in cases) for m in lr.MODES}
        print(f"window {win}: depths {sorted({c.depth for c in cases})}, tracked of {50 * len(cases)}: {tracked}")
        assert min(tracked.values()) >= 10 * len(cases)             # the 5 x 5 grid points inside the frame are 25 of 50


# ---------------------------------------------------------------------------------------------------- 7. gates under the light
@pytest.mark.parametrize("win", lr.GATE_WINDOWS)
def test_every_gate_setting_rejects(pkg, win):
    """Per setting the gate it is about fires at least once: the forward-backward check (lost backwards or too far), and with
    err_max on the cap."""
    scene = lr.gate_scene(pkg, win)
    for gate in lr.gate_settings():
        for mode in lr.MODES:
            stats = np.sum([r["stats"] for r in lr.gated_reference(scene, win, 3, gate, mode)], axis=0)
            print(f"window {win} {mode} {gate}: tracked {stats[0]}, lost backwards {stats[1]}, too far {stats[2]}, over the cap {stats[3]}")
            assert stats[1] + stats[2] >= 1, (win, mode, gate)
            assert gate["err_max"] == 0.0 or stats[3] >= 1, (win, mode, gate)
            assert stats[0] - stats[1:].sum() >= 10, (win, mode, gate)     # and it does not reject everything


# ---------------------------------------------------------------------------------------------------- 8. far coordinates
def test_far_coordinates_are_lost_and_alone(pkg):
    for far, near in lr.far_cases():
        for mode in lr.MODES:
            f, n = far.reference(mode), near.reference(mode)
            rows = [lr.FAR_POINT, *lr.FAR_SEEDS]
            assert not f[1][rows].any() and n[1][rows].all(), (far.tag, mode)
            rest = np.setdiff1d(np.arange(len(f[1])), rows)
            assert all(np.array_equal(bits(a[rest]), bits(b[rest])) for a, b in zip(f, n)), (far.tag, mode)
            assert n[1].mean() >= 0.6
