"""GPU: ofk_lk_pyr_light against the test-side reference (tests/lk_light_reference.py), bit for bit in next, status and err, on every
route of ofk_launch_lk_light (k_lk_light<15>, <21>, <31>), both modes, the seed / eigenvalue flags and three exposures.

The frames are those of tests/test_gpu_lk_seed.py with the next frame under another exposure (synth.apply_exposure) and two
regions painted into it: one constant (vJ = 0: the alpha = 1 branch of rule 4) and one saturated at 255.  Every comparison is
against the reference under the same light; test_the_light_changes_the_tracks shows that the comparison is not vacuous."""
import ctypes as C

import numpy as np
import pytest

import lk_seed_reference as R  # noqa: E402  (tests/lk_seed_reference.py)
import lk_light_reference as LR  # noqa: E402  (tests/lk_light_reference.py)
import track_gate_reference as G  # noqa: E402  (tests/track_gate_reference.py)
from test_gpu_lk_seed import frames, points, seed_kinds, bits  # noqa: E402

pytestmark = pytest.mark.gpu

LK = dict(max_count=20, eps=0.03, min_eig_thr=1e-4)
MODES = ("bias", "gain")
EXPOSURES = [pytest.param((1.0, 0.0, 0.0), id="same"), pytest.param((1.25, 10.0, 0.0), id="brighter"),
             pytest.param((0.75, -5.0, 0.3), id="darker-vignette")]
# (h, w), window, max_level: the small shapes of test_gpu_lk_seed.ROUTES, one per route of the new launcher and the cut pyramids
SHAPES = [
    pytest.param((135, 241), 13, 1, id="light15-w13"), pytest.param((135, 241), 19, 2, id="light21-w19"),
    pytest.param((135, 241), 31, 1, id="light31-w31"), pytest.param((480, 640), 15, 0, id="light15-w15-L0"),
    pytest.param((480, 640), 15, 3, id="light15-w15-L3"), pytest.param((40, 56), 15, 3, id="level-cut-w15"),
    pytest.param((70, 90), 31, 3, id="level-cut-w31"),
]
_scenes = {}


def regions(h, w):
    """(constant, saturated) rectangles (y0, y1, x0, x1) painted into the next frame: each a little larger than a 15 x 15 window."""
    rh, rw = max(h // 5, 12), max(w // 5, 12)
    return (h // 8, h // 8 + rh, w // 8, w // 8 + rw), (h - h // 8 - rh, h - h // 8, w - w // 8 - rw, w - w // 8)


def scene(pkg, h, w, batch, win, exposure, S=72):
    """g0, g1 [B,h,w] with g1 exposed and painted, pts [B,S,2] (test_gpu_lk_seed's mix plus points inside the two regions), truth."""
    key = (h, w, batch, win, tuple(exposure), S)
    if key not in _scenes:
        from of_amd import synth
        g0, g1, base = frames(pkg, h, w, batch)
        g1 = np.stack([synth.apply_exposure(a, *exposure) for a in g1])
        const, sat = regions(h, w)
        g1[:, const[0]:const[1], const[2]:const[3]] = 100
        g1[:, sat[0]:sat[1], sat[2]:sat[3]] = 255
        pts, truth = points(g0, base, S, win, 500 + win)
        extra = np.array([((r[2] + r[3]) / 2 + dx, (r[0] + r[1]) / 2 + dy) for r in (const, sat) for dx, dy in ((0.25, -0.5), (2.0, 1.75))], np.float32)
        pts[:, 12:12 + len(extra)] = extra                      # behind the border points, inside every count of the ragged batches but the last
        truth[:, 12:12 + len(extra)] = extra
        _scenes[key] = (g0, g1, pts, truth)
    return _scenes[key]


def check(ctx, g0, g1, pts, counts, win, L, seed, flags, light, tag, lk=LK):
    got = ctx.lk_pyr(g0, g1, pts, counts, win=win, max_level=L, next_pts=seed, flags=flags, light=light, **lk)
    for b in range(len(g0)):
        n = int(counts[b])
        ref = LR.lk_pyr(g0[b], g1[b], pts[b, :n], win, L, seed=None if seed is None else seed[b, :n], flags=flags, light=light, **lk)
        for name, g, r in zip(("next", "status", "err"), got, ref):
            g = g[b, :n]; r = r.reshape(g.shape)
            assert np.array_equal(bits(g), bits(r)), (tag, light, "image", b, name, int(np.sum(bits(g) != bits(r))), "of", g.size)
    return got


@pytest.mark.parametrize("exposure", EXPOSURES)
@pytest.mark.parametrize("shape,win,L", SHAPES)
def test_lk_pyr_light_matches_reference(pkg, gpu_ctx, shape, win, L, exposure):
    h, w = shape
    B, S = 3, 72
    g0, g1, pts, truth = scene(pkg, h, w, B, win, exposure)
    counts = np.array([S, 41, 5], np.int32)                    # ragged
    noisy = seed_kinds(pts, truth, h, w, 7 * win + L)[1][1]
    for mode in MODES:
        plain = check(gpu_ctx, g0, g1, pts, counts, win, L, None, 0, mode, "plain")
        eig = check(gpu_ctx, g0, g1, pts, counts, win, L, None, R.GET_MIN_EIGENVALS, mode, "eig")
        check(gpu_ctx, g0, g1, pts, counts, win, L, noisy, R.USE_INITIAL_FLOW, mode, "seed")
        check(gpu_ctx, g0, g1, pts, counts, win, L, noisy, R.USE_INITIAL_FLOW | R.GET_MIN_EIGENVALS, mode, "seed+eig")
        for b in range(B):
            n = counts[b]
            assert np.array_equal(bits(eig[0][b, :n]), bits(plain[0][b, :n])) and np.array_equal(eig[1][b, :n], plain[1][b, :n])


def test_the_light_changes_the_tracks(pkg, gpu_ctx):
    """Not a parity statement: under the brighter exposure the three trackers do differ (the comparisons above are not vacuous)."""
    h, w, win = 480, 640, 15
    g0, g1, pts, truth = scene(pkg, h, w, 3, win, (1.25, 10.0, 0.0))
    counts = np.array([72, 72, 72], np.int32)
    off = gpu_ctx.lk_pyr(g0, g1, pts, counts, win=win, max_level=3, **LK)
    bias = gpu_ctx.lk_pyr(g0, g1, pts, counts, win=win, max_level=3, light="bias", **LK)
    gain = gpu_ctx.lk_pyr(g0, g1, pts, counts, win=win, max_level=3, light="gain", **LK)
    assert np.sum(bits(off[0]) != bits(bias[0])) > 100 and np.sum(bits(bias[0]) != bits(gain[0])) > 100
    assert np.sum(bits(bias[2]) != bits(gain[2])) > 50


@pytest.mark.parametrize("shape,win,L", [pytest.param((135, 241), 13, 1, id="w13"), pytest.param((480, 640), 15, 3, id="w15"),
                                        pytest.param((135, 241), 19, 2, id="w19")])
def test_the_clamp_binds(pkg, ofk, gpu_ctx, shape, win, L):
    """A pair six times apart in gain: alpha wants 6 (next frame darker) or 1/6 (previous frame darker), gain_max 4 holds it at 4 or
    1/4.  The clamp is seen to bind: the results under gain_max 4 and 8 differ."""
    from of_amd import synth
    h, w = shape
    B, S = 3, 72
    g0, g1, pts, truth = scene(pkg, h, w, B, win, (1.0, 0.0, 0.0))
    counts = np.array([S, 41, 5], np.int32)
    dark0 = np.stack([synth.apply_exposure(a, 1 / 6.0) for a in g0]); dark1 = np.stack([synth.apply_exposure(a, 1 / 6.0) for a in g1])
    for tag, a, b in (("next-darker", g0, dark1), ("prev-darker", dark0, g1)):
        four = check(gpu_ctx, a, b, pts, counts, win, L, None, 0, ofk.lk_light_setting("gain", 4.0), tag)
        eight = check(gpu_ctx, a, b, pts, counts, win, L, None, 0, ofk.lk_light_setting("gain", 8.0), tag)
        assert np.sum(bits(four[0][0]) != bits(eight[0][0])) > 20, tag
        check(gpu_ctx, a, b, pts, counts, win, L, truth, R.USE_INITIAL_FLOW, ofk.lk_light_setting("gain", 1.5), tag)


@pytest.mark.parametrize("win,L", [(15, 3), (21, 2)])
def test_batch_of_eight_ragged(pkg, ofk, win, L):
    h, w, B, S = 480, 640, 8, 64
    g0, g1, pts, truth = scene(pkg, h, w, B, win, (1.25, 10.0, 0.0), S)
    counts = np.array([S, 0, 1, 63, 4, 5, 33, 17], np.int32)
    ctx = ofk.Context(0, w, h, B, S, 3)
    try:
        for mode in MODES:
            check(ctx, g0, g1, pts, counts, win, L, None, 0, mode, "plain")
            check(ctx, g0, g1, pts, counts, win, L, truth, R.USE_INITIAL_FLOW | R.GET_MIN_EIGENVALS, mode, "seed+eig")
    finally:
        ctx.close()


def _call_light(ofk, ctx, g0, g1, pts, counts, win, L, gate, light, flags=0, init=None):
    B, h, w = g0.shape
    S = pts.shape[1]
    out = dict(next_pts=np.zeros((B, S, 2), np.float32), status=np.zeros((B, S), np.uint8), err=np.zeros((B, S), np.float32),
               back_pts=np.zeros((B, S, 2), np.float32), back_status=np.zeros((B, S), np.uint8), fb2=np.zeros((B, S), np.float32))
    rc = ctx._L.ofk_lk_pyr_light(ctx._h, ofk._p(g0), ofk._p(g1), B, h, w, ofk._p(pts), ofk._p(counts), S, win, L, 20, 0.03, 1e-4,
                                 None if init is None else ofk._p(init), flags, ofk._p(out["next_pts"]), ofk._p(out["status"]), ofk._p(out["err"]),
                                 None if gate is None else C.byref(gate), ofk._p(out["back_pts"]), ofk._p(out["back_status"]), ofk._p(out["fb2"]),
                                 None if light is None else C.byref(light))
    return rc, out


def test_light_off_is_ofk_lk_pyr_fb(pkg, ofk, gpu_ctx):
    """light NULL, or a structure of mode OFF (whatever its gain_max), is ofk_lk_pyr_fb: the same bits in all six outputs."""
    g0, g1, pts, truth = scene(pkg, 480, 640, 3, 15, (1.25, 10.0, 0.0))
    counts = np.array([72, 9, 50], np.int32)
    gate = ofk.track_gate_setting("plain", 0.5)
    for win in (15, 21):
        want = gpu_ctx.lk_pyr_fb(g0, g1, pts, counts, gate, win=win, max_level=3, **LK)
        for light in (None, ofk.LkLight(ofk.LIGHT_OFF, 4.0), ofk.LkLight(ofk.LIGHT_OFF, 0.0)):
            rc, got = _call_light(ofk, gpu_ctx, g0, g1, pts, counts, win, 3, gate, light)
            assert rc == ofk.OK
            for k in want:
                for b in range(3):
                    assert np.array_equal(bits(got[k][b, :counts[b]]), bits(want[k][b, :counts[b]])), (win, k, b)
        via = gpu_ctx.lk_pyr_fb(g0, g1, pts, counts, gate, win=win, max_level=3, light="off", **LK)     # the binding does not reach the new entry
        assert all(np.array_equal(bits(via[k]), bits(want[k])) for k in want)


def test_refusals(pkg, ofk, gpu_ctx):
    g0, g1, pts, truth = scene(pkg, 480, 640, 3, 15, (1.25, 10.0, 0.0))
    counts = np.array([72, 9, 50], np.int32)
    for bad in (ofk.LkLight(3, 4.0), ofk.LkLight(-1, 4.0), ofk.LkLight(ofk.LIGHT_GAIN, 1.0), ofk.LkLight(ofk.LIGHT_BIAS, 0.5),
                ofk.LkLight(ofk.LIGHT_GAIN, np.nan), ofk.LkLight(ofk.LIGHT_GAIN, np.inf)):
        assert _call_light(ofk, gpu_ctx, g0, g1, pts, counts, 15, 3, None, bad)[0] == ofk.E_INVALID, (bad.mode, bad.gain_max)
    on = ofk.lk_light_setting("gain")
    assert _call_light(ofk, gpu_ctx, g0, g1, pts, counts, 15, 3, None, on, flags=16)[0] == ofk.E_INVALID
    assert _call_light(ofk, gpu_ctx, g0, g1, pts, counts, 15, 3, None, on, flags=ofk.LK_USE_INITIAL_FLOW)[0] == ofk.E_INVALID      # no init_pts
    assert gpu_ctx.get_lk_light().mode == ofk.LIGHT_OFF          # the stage entry takes its own setting: the context's stays off
    check(gpu_ctx, g0, g1, pts, counts, 15, 3, None, 0, "gain", "after refusals")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("win,L", [(15, 3), (21, 2)])
def test_gates_run_on_top(pkg, ofk, gpu_ctx, win, L, mode):
    """fb = "plain" with the light on is the reference's composition: forward pass, backward pass under the same light, the gate."""
    g0, g1, pts, truth = scene(pkg, 480, 640, 3, win, (1.25, 10.0, 0.0))
    counts = np.array([72, 41, 5], np.int32)
    gate = G.setting(fb="plain", fb_thr=0.5)
    out = gpu_ctx.lk_pyr_fb(g0, g1, pts, counts, win=win, max_level=L, light=mode, **gate, **LK)
    fired = 0
    for b, c in enumerate(counts):
        r = LR.gated(g0[b], g1[b], pts[b, :c], win, L, gate=gate, light=mode, **LK)
        fired += int(r["stats"][1] + r["stats"][2])
        for k, rk in (("next_pts", "next"), ("status", "status"), ("err", "err"), ("back_pts", "back"), ("back_status", "st_b"), ("fb2", "fb2")):
            assert np.array_equal(bits(out[k][b, :c]), bits(r[rk])), (win, mode, "image", b, k)
    assert fired >= 3                                            # the gate does reject points here
