"""CPU: the test-side reference of the lighting-insensitive LK (tests/lk_light_reference.py) and the exposure experiment behind
ofk_lk_light: the "default" row of lk_seed_reference.ROWS (640 x 480, 300 corners, window 15, maxLevel 3) with the next gray frame
under clip(rint(g1 * gain * f + bias), 0, 255).

Measured here (tracked / wrong / rel / median distance in px / median err of the right points):
    gain, bias, vignette   plain LK                          bias mode                        gain mode
    1,    0,   0           300 /   1 / 0.026  / 0.011 / 2.12  300 / 1 / 0.0088 / 0.012 / 2.10  300 / 1 / 0.0079 / 0.013 / 1.39
    1.25, +10, 0           290 / 146 / 3.94   / 0.50  / 41.0  300 / 1 / 0.0097 / 0.038 / 5.21  300 / 1 / 0.0089 / 0.016 / 1.65
    0.75, -5,  0           251 / 187 / 5.13   / 0.88  / 36.8  300 / 1 / 0.0085 / 0.073 / 8.14  300 / 1 / 0.0080 / 0.014 / 1.41
    1.1,  0,   0           300 /   2 / 0.0053 / 0.156 / 12.4  300 / 1 / 0.0089 / 0.021 / 1.91  300 / 1 / 0.0079 / 0.014 / 1.42
    1.25, +10, 0.3         300 /  63 / 2.87   / 0.29  / 23.7  300 / 1 / 0.0102 / 0.023 / 2.75  300 / 1 / 0.0081 / 0.016 / 1.52
The err rule (rule 6): the median err of the right points goes from 2.12 to 41.0 under the 25 % step with the plain tracker, from
2.10 to 5.21 in bias mode (the offset is taken out, the gain is not) and from 1.39 to 1.65 in gain mode - so an err_max chosen on
unchanged exposure keeps its meaning in gain mode.  Row "yaw0.08": 286 right points on unchanged exposure, 285 (bias) / 286 (gain)
at (1.25, +10), 100 with the plain tracker."""
import numpy as np
import pytest

import lk_seed_reference as R  # noqa: E402  (tests/lk_seed_reference.py)
import lk_light_reference as LR  # noqa: E402  (tests/lk_light_reference.py)

LIGHTS = (None, "bias", "gain")
_table = {}


def table():
    """Every row of the experiment under every tracker, computed once and printed."""
    if not _table:
        for ex in LR.EXPOSURES:
            for light in LIGHTS:
                _table[ex, light] = LR.experiment_row("default", ex, light)
        print("\ngain bias vignette | tracker: tracked wrong right rel median-dist median-err")
        for ex in LR.EXPOSURES:
            for light in LIGHTS:
                r = _table[ex, light]
                print(f"{ex[0]:5.2f} {ex[1]:5.1f} {ex[2]:4.1f} | {light or 'plain':5s}: {r['tracked']:3d} {r['wrong']:3d} {r['right']:3d} {r['rel']:.4f} "
                      f"{r['dist']:.4f} {r['err']:.3f}")
    return _table


@pytest.mark.parametrize("flags", [0, R.GET_MIN_EIGENVALS, R.USE_INITIAL_FLOW, R.USE_INITIAL_FLOW | R.GET_MIN_EIGENVALS])
@pytest.mark.parametrize("win,L", [(15, 3), (21, 1), (9, 2)])
def test_mode_off_is_the_seeded_reference(pkg, win, L, flags):
    e = R.experiment_pair("default")
    g1 = LR.exposed_g1("default", (1.25, 10.0, 0.3))
    pts = e["pts"][:120]
    seed = (pts + np.float32(1.5)).astype(np.float32)
    want = R.lk_pyr(e["g0"], g1, pts, win, L, seed=seed, flags=flags)
    for light in (None, "off", (LR.OFF, 0.0)):
        got = LR.lk_pyr(e["g0"], g1, pts, win, L, seed=seed, flags=flags, light=light)
        for g, w in zip(got, want):
            assert np.array_equal(g.view(np.uint8), w.view(np.uint8))


def test_plain_lk_breaks_under_an_exposure_step(pkg):
    t = table()
    for ex in LR.EXPOSURES[1:3]:
        r = t[ex, None]
        assert r["wrong"] / r["tracked"] >= 0.30, (ex, r)


@pytest.mark.parametrize("light", ["bias", "gain"])
def test_compensation_repairs_every_row(pkg, light):
    t = table()
    for ex in LR.EXPOSURES:
        r = t[ex, light]
        assert r["wrong"] <= 3 and r["right"] >= 297 and r["rel"] <= 0.02, (ex, light, r)


def test_gain_mode_is_closer_than_bias_mode(pkg):
    t = table()
    for ex in LR.EXPOSURES[1:3]:
        assert t[ex, "gain"]["dist"] < 0.5 * t[ex, "bias"]["dist"], (ex, t[ex, "gain"], t[ex, "bias"])


@pytest.mark.parametrize("light", ["bias", "gain"])
def test_large_motion_row_under_an_exposure_step(pkg, light):
    same = LR.experiment_row("yaw0.08", (1.0, 0.0, 0.0), None)
    r = LR.experiment_row("yaw0.08", (1.25, 10.0, 0.0), light)
    plain = LR.experiment_row("yaw0.08", (1.25, 10.0, 0.0), None)
    print(f"\nyaw0.08: right points {same['right']} on unchanged exposure, {r['right']} in {light} mode and {plain['right']} plain at (1.25, +10)")
    assert r["right"] >= 0.95 * same["right"], (r, same)


def test_err_keeps_its_meaning_in_gain_mode(pkg):
    """Rule 6: the figures are in the module docstring and printed here.  What is asserted is the order the rule implies, not the
    figures: under an exposure step the residual with the offset taken out is below the plain one, and the one with gain and
    offset taken out is below that."""
    t = table()
    same, step = LR.EXPOSURES[0], LR.EXPOSURES[1]
    print("\nmedian err of the right points, unchanged exposure -> (1.25, +10): " +
          ", ".join(f"{light or 'plain'} {t[same, light]['err']:.3f} -> {t[step, light]['err']:.3f}" for light in LIGHTS))
    assert t[step, "gain"]["err"] < t[step, "bias"]["err"] < t[step, None]["err"]


def test_bias_mode_does_not_read_gain_max(pkg):
    e = R.experiment_pair("default")
    g1 = LR.exposed_g1("default", (1.25, 10.0, 0.0))
    a = LR.lk_pyr(e["g0"], g1, e["pts"], light=(LR.BIAS, 4.0)); b = LR.lk_pyr(e["g0"], g1, e["pts"], light=(LR.BIAS, 1.0001))
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
    c = LR.lk_pyr(e["g0"], g1, e["pts"], light=(LR.GAIN, 4.0)); d = LR.lk_pyr(e["g0"], g1, e["pts"], light=(LR.GAIN, 1.0001))
    assert not np.array_equal(c[0].view(np.uint8), d[0].view(np.uint8))      # the clamp at 1.0001 binds at gain 1.25
    with pytest.raises(ValueError):
        LR.lk_pyr(e["g0"], g1, e["pts"], light=(LR.GAIN, 1.0))
