"""CPU: the restatement of the track templates (tests/track_template_reference.py; include/ofk.h: ofk_set_track_template) on analytic
cases, and the experiment behind the feature: the C oracle's LK chain over three rendered sequences (480 x 640, seed 5, 300 corners at
quality 0.01 / min_distance 10 / block 3, window 15, maxLevel 3, 30 frames, no re-detection) with the restatement behind every LK step,
against the truth H^k(birth position).

Every test of this file exercises the numpy restatement and the C oracle alone, so all of them pass on the parent commit as well: they
hold the rules and the experiment, not the library.  The tests that need the feature are tests/test_track_template_abi.py and
tests/test_gpu_track_template.py.

Measured here at step 29, median / p90 drift in px, tracks within 0.5 px of the tracks alive:
                LK alone                 LK + score (anchor_iters 0)   templates on (defaults)
    yaw         0.946 / 1.625, 34 / 234  0.886 / 1.351, 34 / 205       0.012 / 0.034, 227 / 235
    climb       0.421 / 0.823, 186 / 300 0.420 / 0.817, 186 / 299      0.019 / 0.038, 300 / 300
    fast        1.343 / 2.356, 4 / 47    1.092 / 2.052, 4 / 27         0.044 / 0.525, 43 / 48
On climb all 300 templated tracks are alive at step 29 (the lowest score 0.992).
Recorded, not asserted (test_scores_outside_rows_and_sixty_frames prints them):
  scores       with the setting on, runs at ncc_min 0.8 and at 0.9 keep the same rows at the same positions after every one of the 29
               steps in all three sequences: the lowest score of any kept row at any step is 0.996 (yaw) / 0.992 (climb) / 0.981
               (fast), the tracks within 0.5 px at step 29 score at least 0.997 / 0.983, and no scored track is beyond 1.5 px.
               With the score alone (anchor_iters 0) the drift is not corrected and the threshold matters: at 0.8 yaw keeps 205
               tracks, 33 scored ones within 0.5 px (lowest 0.978) and 8 beyond 1.5 px (0.816-0.947); at 0.9 it keeps 150, the
               same 33 and 3 beyond 1.5 px (0.907-0.947); fast keeps 27 / 14, 3 within 0.5 px (0.963) and 1 / 0 beyond 1.5 px
               (0.847): a drifted track can score above 0.9, so the score alone does not separate them.
  outside      every track beyond 1.5 px with the setting on is an OUTSIDE row (its window has left the frame: 1 in yaw, 3 in fast)
               or a NO_TEMPLATE row (born with its rim outside: 1 in yaw); outside = drop leaves 0.010 / 0.025, 217 / 220 (yaw; the
               one left is the NO_TEMPLATE row, 3.3 px off) and 0.040 / 0.064, 40 / 40 (fast, largest 0.24 px).
  60 frames    climb: 0.019 / 0.038 at step 29, 0.024 / 0.048 at 45, 0.023 / 0.048 at 59, 300 of 300 alive within 0.5 px throughout.
"""
import functools

import numpy as np
import pytest

import track_template_reference as T

F = np.float32


def smooth(h, w, dx=0.0, dy=0.0, rot=0.0, scale=1.0, c=None):
    """An analytic texture (waves of 9-23 px) seen through x' = c + s R (x - c) + d, rounded to u8: the content at x in the
    undeformed image is at x' in this one."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = (w / 2.0, h / 2.0) if c is None else c
    ux, uy = xx - dx - cx, yy - dy - cy                          # back through the map
    co, si = np.cos(rot) / scale, np.sin(rot) / scale
    sx, sy = co * ux + si * uy + cx, -si * ux + co * uy + cy
    v = 128 + 40 * np.sin(sx / 3.7 + 0.3) * np.cos(sy / 2.9) + 35 * np.sin((sx + sy) / 2.3 + 1.0) + 30 * np.cos((sx - 2 * sy) / 3.1)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("shift", [0.3, 1.0, 1.9])
def test_a_shifted_patch_comes_back(shift):
    cfg = T.setting()
    g0, d = smooth(64, 80), (shift, -0.5 * shift)
    g1 = smooth(64, 80, *d)
    t = T.capture(g0, 40, 32, cfg.win)
    p, ncc, flag, drop = T.score_row(g1, (40, 32), np.array([1, 0, 0, 1], F), t, cfg)      # "LK" has not moved at all
    assert flag == T.PASS and not drop and ncc > 0.99
    assert abs(p[0] - (40 + d[0])) < 0.05 and abs(p[1] - (32 + d[1])) < 0.05, (p, d)


def test_a_shift_beyond_anchor_max_is_abandoned():
    cfg = T.setting(ncc_min=-1.0)
    g0, g1 = smooth(64, 80), smooth(64, 80, 2.5, 0.0)
    t = T.capture(g0, 40, 32, cfg.win)
    p, ncc, flag, drop = T.score_row(g1, (40, 32), np.array([1, 0, 0, 1], F), t, cfg)
    assert flag == T.ABANDONED and not drop and tuple(p) == (40, 32)
    p0, ncc0, _, _ = T.score_row(g1, (40, 32), np.array([1, 0, 0, 1], F), t, T.setting(ncc_min=-1.0, anchor_iters=0))
    assert ncc == ncc0                                           # scored at LK's position


def test_a_rotated_and_scaled_patch_needs_the_accumulated_map():
    cfg = T.setting(anchor_iters=0)
    g0 = smooth(96, 96)
    g1 = smooth(96, 96, rot=0.6, scale=1.4, c=(48.0, 48.0))
    t = T.capture(g0, 48, 48, cfg.win)
    A = (1.4 * np.array([np.cos(0.6), -np.sin(0.6), np.sin(0.6), np.cos(0.6)])).astype(F)
    _, ncc, flag, _ = T.score_row(g1, (48, 48), A, t, cfg)
    assert flag == T.PASS and ncc > 0.95, ncc
    _, ncc_i, flag_i, drop = T.score_row(g1, (48, 48), np.array([1, 0, 0, 1], F), t, cfg)
    assert ncc_i < 0.8 and flag_i == T.FAIL and drop, ncc_i


def test_a_constant_patch_is_flat_and_an_edge_has_no_anchor():
    cfg = T.setting()
    g = np.full((48, 64), 90, np.uint8)
    t = T.capture(g, 30, 20, cfg.win)
    assert T.score_row(smooth(48, 64), (30, 20), np.array([1, 0, 0, 1], F), t, cfg)[2] == T.FLAT       # vT = 0
    assert T.score_row(g, (30, 20), np.array([1, 0, 0, 1], F), T.capture(smooth(48, 64), 30, 20, cfg.win), cfg)[2] == T.FLAT   # vJ = 0
    edge = np.repeat((np.arange(64) * 3).astype(np.uint8)[None], 48, 0)     # a pure horizontal ramp: det = 0, no anchor
    p, ncc, flag, _ = T.score_row(edge, (30.4, 20), np.array([1, 0, 0, 1], F), T.capture(edge, 30, 20, cfg.win), cfg)
    assert flag == T.PASS and tuple(p) == (F(30.4), F(20)) and ncc > 0.99
    assert T.capture(g, 7.5, 20, cfg.win) is None and T.capture(g, 8, 20, cfg.win) is not None          # the rim needs x - 8 >= 0
    assert T.score_row(g, (6.5, 20), np.array([1, 0, 0, 1], F), t, cfg)[2:] == (T.OUTSIDE, False)
    assert T.score_row(g, (6.5, 20), np.array([1, 0, 0, 1], F), t, T.setting(outside=T.DROP))[2:] == (T.OUTSIDE, True)


def test_the_sampler_rounds_the_fraction_to_even_and_refuses_what_is_no_number():
    g = smooth(16, 16)
    o = np.array([0])
    v, out = T.sample(g, 3 + 1.5 / 32, 4 + 2.5 / 32, (1, 0, 0, 1), o, o)    # frac * 32 = 1.5 -> 2, 2.5 -> 2
    I = g.astype(np.int64)
    assert not out[0] and v[0] == I[4, 3] * 30 * 30 + I[4, 4] * 2 * 30 + I[5, 3] * 30 * 2 + I[5, 4] * 2 * 2
    for p in ((np.nan, 4), (3, np.inf), (-0.01, 4), (15.0, 4), (3, 15.5)):
        assert T.sample(g, p[0], p[1], (1, 0, 0, 1), o, o)[1][0], p
    assert not T.sample(g, 14.99, 14, (1, 0, 0, 1), o, o)[1][0]
    assert T.sample(g, 3, 4, (np.nan, 0, 0, 1), o + 1, o)[1][0]


def test_the_step_map_recovers_a_similarity_and_sheds_outliers():
    rng = np.random.default_rng(3)
    prev = (rng.random((200, 2)) * (640, 480)).astype(F)
    c, M, t = np.array([320.0, 240.0]), 1.01 * np.array([[np.cos(0.02), -np.sin(0.02)], [np.sin(0.02), np.cos(0.02)]]), np.array([1.5, -0.7])
    nxt = ((prev - c) @ M.T + t + c).astype(F)
    st = np.ones(200, np.uint8)
    few = nxt.copy(); few[:6] += 20                                  # 3 % of the rows 20 px off: the first fit is 0.85 px off, the second sheds them
    rec, L = T.affine_fit(prev, few, st, 200, 480, 640, T.setting())
    assert rec[6] == 0 and rec[7] == 200 and 150 <= rec[8] <= 194 and np.allclose(rec[0:4], M.ravel(), atol=1e-6) and np.allclose(rec[4:6], t, atol=1e-4)
    assert rec[9] < 1e-4 and L.dtype == F
    rec1, _ = T.affine_fit(prev, few, st, 200, 480, 640, T.setting(fit_gate=0.0))
    assert rec1[8] == 0 and abs(rec1[4] - t[0]) > 0.5 and rec1[9] > 1
    many = nxt.copy(); many[:60] += 20                               # 30 %: the first fit is 8.5 px off for every row, nothing lies inside 2 px of it
    rec2, _ = T.affine_fit(prev, many, st, 200, 480, 640, T.setting())
    assert rec2[6] == 0 and rec2[8] == 0 and abs(rec2[4] - t[0]) > 5  # ... and the first fit stands: the gate is no robust estimator
    line = np.column_stack([np.arange(50.0), 2 * np.arange(50.0)]).astype(F)
    assert T.affine_fit(line, line, st[:50], 50, 480, 640, T.setting())[0][6] == 1            # collinear: the identity
    assert T.affine_fit(prev, nxt, st, 5, 480, 640, T.setting())[0][6] == 1                   # fewer than fit_min


# ---------------------------------------------------------------------------------------------------------------- the experiment
@functools.lru_cache(None)
def run(name, kind, n_frames=30):
    cfg = {"lk": None, "score": T.setting(anchor_iters=0), "on": T.setting(), "drop": T.setting(outside=T.DROP), "on09": T.setting(ncc_min=0.9),
           "score09": T.setting(anchor_iters=0, ncc_min=0.9)}[kind]
    return T.run_sequence(name, cfg, n_frames)


@pytest.mark.parametrize("name", list(T.SEQUENCES))
def test_templates_hold_the_drift_of_thirty_frames(name):
    on, lk, score = (T.summary(run(name, k)[-1]) for k in ("on", "lk", "score"))
    print(f"{name}: LK alone {lk}, LK + score {score}, templates on {on}")
    assert on[0] <= 0.1
    assert on[0] <= 0.2 * lk[0] and on[0] <= 0.2 * score[0]
    assert on[2] > lk[2] and on[3] >= score[3]                   # more tracks within 0.5 px, no fewer alive than with the score alone


def test_climb_loses_no_track_that_stays_inside():
    on, lk = run("climb", "on"), run("climb", "lk")
    truth_inside = on[-1]["inside"]
    assert len(on[-1]["err"]) == len(lk[-1]["err"]) == T.CORNERS and truth_inside.all()      # every window stays inside; none is dropped
    assert (on[-1]["flag"] & 15 == T.PASS).all() and on[-1]["ncc"].min() >= 0.92


def test_scores_outside_rows_and_sixty_frames():
    for name in ("yaw", "fast"):
        s = run(name, "on")[-1]
        v, e = s["flag"] & 15, s["err"]
        scored = np.isin(v, (T.PASS, T.ABANDONED))
        good, bad = scored & (e <= 0.5), scored & (e > 1.5)
        print(f"{name}: within 0.5 px {good.sum()} rows, lowest score {s['ncc'][good].min():.4f} (0.8 drops {(s['ncc'][good] < 0.8).sum()}, "
              f"0.9 drops {(s['ncc'][good] < 0.9).sum()}); beyond 1.5 px scored {bad.sum()}, not scored {(~scored & (e > 1.5)).sum()} with flags "
              f"{sorted(set(v[~scored & (e > 1.5)]))}")
        hi = run(name, "on09")
        print(f"{name}: ncc_min 0.9 against 0.8, the same rows at the same positions after every step: "
              f"{all(np.array_equal(a['pts'], b['pts']) for a, b in zip(run(name, 'on'), hi))}; step 29 {T.summary(hi[-1])}")
        for kind in ("score", "score09"):
            c = run(name, kind)[-1]
            cs = np.isin(c["flag"] & 15, (T.PASS, T.ABANDONED))
            cg, cb = cs & (c["err"] <= 0.5), cs & (c["err"] > 1.5)
            print(f"{name}, {kind}: {T.summary(c)}; within 0.5 px {cg.sum()} (lowest score {c['ncc'][cg].min() if cg.any() else None}), "
                  f"beyond 1.5 px {cb.sum()} (scores {(c['ncc'][cb].min(), c['ncc'][cb].max()) if cb.any() else None})")
        d = run(name, "drop")[-1]
        print(f"{name}: outside = drop {T.summary(d)}, beyond 1.5 px {(d['err'] > 1.5).sum()}, largest {d['err'].max():.3f}")
        assert s["ncc"][good].min() >= 0.92                      # what the issue's sketch saw of the tracks within 0.5 px
    long = run("climb", "on", 60)
    for k in (28, 44, 58):
        print(f"climb, 60 frames, step {k + 1}: {T.summary(long[k])}")
