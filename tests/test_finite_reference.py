"""The finite motion on the CPU (tests/finite_reference.py, the numpy restatement of include/ofk.h): what taking a frame pair for the
instantaneous motion field costs the velocity solve, and that the rewrite of the two point sets gives all of it back - the oracle's
own NODE and SIM solves on the rewritten points return the displacement T of P1 = R P0 + T.

Bounds.  Without rounding the rewrite is an identity of the plane's geometry: 1e-9 leaves room for the conditioning of a 1200 x 3
system over the 4e-16 .. 3e-14 measured.  With one float32 rounding of every pixel coordinate (below 2048: at most 1.2e-4 px,
against flows of 5 px and more, averaged over 400 points): 1e-5 over the 4e-9 .. 1.4e-6 measured.  The plain solve's error on the
same points reproduces the table of the feature's proposal within 10 % of each figure.

Joint, plane and robust references on raw and on rewritten points, 0.2 px of flow noise, seed 23 (|v - T| / |T|; printed by
test_joint_plane_and_robust_references_on_rewritten_points):
                 row 2 raw   row 2 rewritten   row 4 raw   row 4 rewritten
    robust       0.02896     0.00058           0.18291     0.00025
    joint        0.02026     0.00151           0.24664     0.00160
    plane        0.02497     0.00055           0.18290     0.00036
(joint: every axis of omega free; plane: the tilt free.)  Neither the joint nor the plane solve is worse with the rewrite at either
motion: on raw points their extra unknowns absorb little of the finite motion's error (the joint solve at row 4 even adds to the plain
solve's 0.183), on rewritten points they stay within three times the plain solve's noise floor."""
import hashlib

import numpy as np
import pytest

import finite_reference as F
import joint_reference as J
import plane_reference as P
import robust_reference as RR

NOISE_PX = 0.2
_cache = {}


def case(i):
    """(scene, sensor row, previous pixels, next pixels) of motion i, float64, computed once."""
    if i not in _cache:
        m = F.MOTIONS[i]
        sc = F.exact_scene(m["T"], m["omega"])
        sr = F.sensor_row(sc)
        _cache[i] = sc, sr, F.to_px(sc["x0"], sr), F.to_px(sc["x1"], sr)
    return _cache[i]


def noisy(i, seed=23):
    sc, sr, p0, p1 = case(i)
    rng = np.random.default_rng(seed + i)
    return sc, sr, p0, p1 + rng.normal(0.0, NOISE_PX, p1.shape)


@pytest.mark.parametrize("i", range(5))
@pytest.mark.parametrize("variant", ["node", "sim"])
def test_rewritten_points_give_the_displacement_exactly(i, variant):
    sc, sr, p0, p1 = case(i)
    a, b, good = F.correct_f64(F.setting(), p0, p1, sr[None])
    assert good.all()
    v = F.solve_points(a, b, sr, variant)
    flow = float(np.abs(sc["x1"] - sc["x0"]).max())
    err = F.error(v, sc["T"])
    print(i, variant, "rewritten, f64:", err)
    if i == 4:
        assert err < 1e-9 * flow                                 # pure rotation: no velocity at all
    else:
        assert err < 1e-9


@pytest.mark.parametrize("i", range(5))
def test_rewritten_points_rounded_to_f32(i):
    sc, sr, p0, p1 = case(i)
    a, b, good = F.correct_points(F.setting(), p0.astype(np.float32), p1.astype(np.float32), sr[None], full=True)
    assert good.all() and a.dtype == np.float32 and b.dtype == np.float32
    err = F.error(F.solve_points(a, b, sr), sc["T"])
    print(i, "rewritten, f32 pixels:", err)
    assert err < 1e-5


@pytest.mark.parametrize("i", range(5))
def test_plain_solve_reproduces_the_table(i):
    sc, sr, p0, p1 = case(i)
    m = F.MOTIONS[i]
    err = F.error(F.solve_points(p0, p1, sr), sc["T"])
    flow = F.max_flow_px(sc, sr)
    print(i, "largest flow", flow, "px; plain:", err, "table:", m["plain"])
    assert abs(err - m["plain"]) <= 0.10 * m["plain"]


def test_with_noise_the_rewrite_is_no_worse_than_the_plain_solve_plus_the_floor():
    res = []
    for i in range(5):
        sc, sr, p0, p1 = noisy(i)
        a, b, good = F.correct_points(F.setting(), p0.astype(np.float32), p1.astype(np.float32), sr[None], full=True)
        assert good.all()
        res.append((F.error(F.solve_points(p0, p1, sr), sc["T"]), F.error(F.solve_points(a, b, sr), sc["T"])))
        print(i, "0.2 px of noise: plain", res[-1][0], "rewritten", res[-1][1])
    floor = res[0][1]                                            # row 1 is the noise floor: its finite-motion error is below it
    floor_abs = floor * np.linalg.norm(F.MOTIONS[0]["T"])        # row 5 has no |T| to divide by
    for i, (plain, fin) in enumerate(res):
        assert fin <= plain + (floor_abs if i == 4 else floor), (i, plain, fin, floor)
    for i in (1, 2, 3):                                          # where the finite motion dominates, the rewrite removes it
        assert res[i][1] < 0.1 * res[i][0]


def test_first_order_limit():
    """At omega = 0 the rewrite moves the position by the flow (x^ = p0) and changes the flow by (s - 1) u: as T -> 0 both vanish
    against the flow, the second one quadratically.  At T = 0 nothing moves, to the bit."""
    m = F.MOTIONS[1]
    ratios = []
    for k in (1e-1, 1e-2, 1e-3):
        sc = F.exact_scene(np.array(m["T"]) * k, (0.0, 0.0, 0.0))
        sr = F.sensor_row(sc)
        p0, p1 = F.to_px(sc["x0"], sr), F.to_px(sc["x1"], sr)
        a, b, good = F.correct_f64(F.setting(), p0, p1, sr[None])
        assert good.all()
        x, u = F.xu(p0, p1, sr); xh, uh = F.xu(a, b, sr)
        assert np.abs(xh - x).max() <= np.abs(u).max() * (1 + 1e-9)
        ratios.append(np.abs(uh - u).max() / np.abs(u).max())
        assert ratios[-1] <= 2.0 * np.linalg.norm(m["T"]) * k    # |s - 1| = |n.T| / |n.P1| <= |T| / (d - |T|)
    assert ratios[1] < 0.2 * ratios[0] and ratios[2] < 0.2 * ratios[1]
    sc = F.exact_scene((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    sr = F.sensor_row(sc)
    p = F.to_px(sc["x0"], sr).astype(np.float32)
    a, b, good = F.correct_points(F.setting(), p, p, sr[None], full=True)
    assert good.all() and np.array_equal(a, p) and np.array_equal(b, p)


# ---------------------------------------------------------------------------------------------------- fallbacks
def _one(prev, nxt, sr, **kw):
    a, b, good = F.correct_points(F.setting(**kw), np.array([prev], np.float32), np.array([nxt], np.float32), sr[None], full=True)
    return a[0], b[0], bool(good[0])


def _row(n=(0.0, 0.0, 1.0), om=(0.0, 0.0, 0.0), sc=1.0 / 800, c=(640.0, 480.0)):
    sr = np.zeros(28)
    sr[0] = 1.0; sr[1:4] = n; sr[4:7] = om; sr[19] = sc; sr[20:22] = c
    return sr


def test_a_usual_point_is_rewritten():
    a, b, good = _one((700.0, 500.0), (720.0, 490.0), _row(om=(0.01, -0.02, 0.03)))
    assert good and not np.array_equal(b, np.float32([720.0, 490.0]))


def test_fallback_scaling_zero():
    a, b, good = _one((700.0, 500.0), (720.0, 490.0), _row(om=(0.01, -0.02, 0.03), sc=0.0))
    assert not good and np.array_equal(a, np.float32([700.0, 500.0])) and np.array_equal(b, np.float32([720.0, 490.0]))


def test_fallback_depth_below_min_depth():
    sr = _row(om=(0.0, 1.5, 0.0))                                # the centre point turns to a depth of cos(1.5) = 0.07
    a, b, good = _one((640.0, 480.0), (700.0, 480.0), sr)
    assert not good and np.array_equal(a, np.float32([640.0, 480.0])) and np.array_equal(b, np.float32([700.0, 480.0]))
    assert _one((640.0, 480.0), (700.0, 480.0), sr, min_depth=0.05)[2]         # the threshold is the setting's
    sr = _row(om=(0.0, 2.0, 0.0))                                # behind the camera
    assert not _one((640.0, 480.0), (700.0, 480.0), sr, min_depth=1e-6)[2]


def test_fallback_next_point_on_the_planes_horizon():
    sr = _row(n=(1.0, 0.0, 0.0))                                 # n.p1 = x1 = 0
    a, b, good = _one((700.0, 500.0), (640.0, 490.0), sr)
    assert not good and np.array_equal(a, np.float32([700.0, 500.0])) and np.array_equal(b, np.float32([640.0, 490.0]))
    sr[1:4] = np.nan
    assert not _one((700.0, 500.0), (720.0, 490.0), sr)[2]


def test_fallback_plane_factor_not_positive():
    sr = _row(n=(1.0, 0.0, 0.0))                                 # n.q~ < 0 < n.p1: the two ends on either side of the horizon
    a, b, good = _one((600.0, 500.0), (700.0, 490.0), sr)
    assert not good and np.array_equal(a, np.float32([600.0, 500.0])) and np.array_equal(b, np.float32([700.0, 490.0]))


def test_fallback_result_not_finite_or_beyond_1e6():
    sr = _row(om=(0.0, np.pi / 2 - 1e-5, 0.0))                   # depth 1e-5 >= min_depth 1e-6: a = 1e5, 8e7 px
    a, b, good = _one((640.0, 480.0), (700.0, 480.0), sr, min_depth=1e-6)
    assert not good and np.array_equal(a, np.float32([640.0, 480.0])) and np.array_equal(b, np.float32([700.0, 480.0]))
    a, b, good = _one((np.nan, 480.0), (700.0, 480.0), _row(om=(0.01, 0.0, 0.0)))
    assert not good and np.isnan(a[0]) and np.array_equal(b, np.float32([700.0, 480.0]))
    a, b, good = _one((np.inf, 480.0), (700.0, 480.0), _row(om=(0.01, 0.0, 0.0)))
    assert not good and np.isinf(a[0])


# ---------------------------------------------------------------------------------------------------- synth
LINEAR_SHA256 = "9acc4d3299baf8e8996edaa9aa68c89bb5223f3d46b33d2f37e739f35ad888bf"      # render_pair(48, 64, 3) before the option existed


def test_synth_finite_agrees_with_the_scene_and_linear_is_unchanged(pkg):
    from of_amd import synth
    for i in (1, 3):
        sc, sr, p0, p1 = case(i)
        H = synth.pixel_homography(sc["T"], sc["omega"], sc["d1"], sc["n1"], sr[19], sr[20], sr[21], motion="finite")
        q = np.concatenate([p0, np.ones((len(p0), 1))], 1) @ H.T
        assert np.abs(q[:, :2] / q[:, 2:3] - p1).max() < 1e-9      # pixels
        Hl = synth.pixel_homography(sc["T"], sc["omega"], sc["d1"], sc["n1"], sr[19], sr[20], sr[21])
        assert np.array_equal(Hl, synth.pixel_homography(sc["T"], sc["omega"], sc["d1"], sc["n1"], sr[19], sr[20], sr[21], motion="linear"))
        assert np.abs(Hl - H).max() > 1e-6
    r = synth.render_pair(48, 64, 3)
    assert hashlib.sha256(r["prev"].tobytes() + r["next"].tobytes() + r["H"].tobytes()).hexdigest() == LINEAR_SHA256
    f = synth.render_pair(48, 64, 3, motion="finite")
    assert np.array_equal(f["prev"], r["prev"]) and not np.array_equal(f["H"], r["H"])
    fr, info = synth.render_sequence(48, 64, 3, 3, motion="finite")
    assert np.array_equal(info["H"], f["H"]) and fr.shape == (3, 48, 64, 3)
    with pytest.raises(ValueError):
        synth.pixel_homography((0, 0, 0), (0, 0, 0), 1.0, (0, 0, 1), 1.0, 0, 0, motion="exact")
    from of_amd.pipeline import RollingShutter
    with pytest.raises(ValueError):
        synth.render_pair(48, 64, 3, rolling_shutter=RollingShutter(readout=0.5), motion="finite")


# ---------------------------------------------------------------------------------------------------- the other solves
def test_joint_plane_and_robust_references_on_rewritten_points():
    """The figures of this module's docstring.  The robust solve must not lose by the rewrite; the joint and the plane solve are
    recorded (the rewrite uses the uncorrected omega and n: an error of second order, correction x flow, is expected there)."""
    sf = NOISE_PX / F.FOCAL
    for i in (1, 3):
        sc, sr, p0, p1 = noisy(i)
        a, b, good = F.correct_points(F.setting(), p0.astype(np.float32), p1.astype(np.float32), sr[None], full=True)
        assert good.all()
        out = {}
        for name, (q0, q1) in (("raw", (p0, p1)), ("rewritten", (a, b))):
            x, u = F.xu(q0, q1, sr)
            rob = RR.robust_solve(RR.NODE, x, u, sr[0], sr[1:4], sr[4:7], seed=5)
            jo = J.joint_solve(J.NODE, x, u, sr[0], sr[1:4], sr[4:7], sf, (np.inf, np.inf, np.inf))
            pl = P.plane_solve(P.NODE, x, u, sr[0], sr[1:4], sr[4:7], sf, np.inf)
            out[name] = dict(robust=F.error(rob["v"], sc["T"]), joint=F.error(jo["v"], sc["T"]), plane=F.error(pl["v"], sc["T"]),
                             joint_flag=jo["flag"], plane_flag=pl["flag"])
        print("row", i + 1, out)
        assert out["rewritten"]["robust"] <= out["raw"]["robust"]
        assert out["rewritten"]["joint_flag"] == 0 and out["rewritten"]["plane_flag"] == 0
        assert all(np.isfinite(out[k][s]) for k in out for s in ("joint", "plane"))
