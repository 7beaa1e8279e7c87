"""Inputs of tests/test_gpu_lk_light_ranges.py (the lighting-insensitive LK over its window and parameter range) and of
tests/test_lk_light_ranges_reference.py, which shows from the reference alone that every one of them keeps the tracker live.
A restatement of ofk_launch_lk_light's routing, one builder per section of the GPU file and the numpy restatement of the 32-bit
row sums of k_lk_light<15>.  Test infrastructure only: numpy, the CPU oracle and tests/lk_light_reference.py, no GPU."""
import itertools

import numpy as np

import param_ranges as pr
import lk_seed_reference as R  # tests/lk_seed_reference.py
import lk_light_reference as LR  # tests/lk_light_reference.py
import track_gate_reference as G  # tests/track_gate_reference.py
from oracle import image_oracle as io
from test_gpu_param_ranges import (WINDOWS, LK_GEOMS, LK_GEOMS_15, CRIT_MAX_COUNT, CRIT_EPS, CRIT_MIN_EIG, border_points,
                                   corner_points, gray_pair)
from test_gpu_lk_seed import frames, points

MODES = ("bias", "gain")
EXPOSURE = (1.25, 10.0, 0.0)                     # gain, bias, vignette of the brighter next frame
SEED_EIG = R.USE_INITIAL_FLOW | R.GET_MIN_EIGENVALS
LIGHT_KERNELS = {"k_lk_light<15>", "k_lk_light<21>", "k_lk_light<31>"}
LK = dict(max_count=20, eps=0.03, min_eig_thr=1e-4)


def light_kernel(win):
    """k_lk.hip launch_lk_light_flagged: the window alone decides."""
    return "k_lk_light<15>" if win <= 15 else "k_lk_light<21>" if win <= 21 else "k_lk_light<31>"


class Case:
    """One call of ofk_lk_pyr_light: frames [B,h,w], points [B,S,2], counts [B], the seed (or None), the flags and the criteria."""

    def __init__(self, tag, g0, g1, pts, win, L, seed=None, flags=0, counts=None, lk=LK, **extra):
        g0 = np.ascontiguousarray(g0, np.uint8); g1 = np.ascontiguousarray(g1, np.uint8)
        pts = np.ascontiguousarray(pts, np.float32)
        if g0.ndim == 2:                                        # one image: a batch of one
            g0, g1, pts = g0[None], g1[None], pts[None]
            seed = None if seed is None else np.ascontiguousarray(seed, np.float32)[None]
        self.tag, self.g0, self.g1, self.pts, self.win, self.L, self.seed, self.flags, self.lk = tag, g0, g1, pts, win, L, seed, flags, dict(lk)
        self.counts = np.full(len(g0), pts.shape[1], np.int32) if counts is None else np.asarray(counts, np.int32)
        self.__dict__.update(extra)

    def reference(self, light, b=0, iters=False):
        """tests/lk_light_reference.lk_pyr on image b -> (next [n,2], status [n], err [n][, Newton steps [n,9]])."""
        n = int(self.counts[b])
        r = LR.lk_pyr(self.g0[b], self.g1[b], self.pts[b, :n], self.win, self.L, seed=None if self.seed is None else self.seed[b, :n],
                      flags=self.flags, light=light, iters=iters, **self.lk)
        return (r[0].reshape(n, 2), r[1].ravel(), r[2].ravel()) + tuple(r[3:])


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def exposed_pair(h, w, seed):
    """gray_pair(h, w, seed) -> (previous frame, next frame under EXPOSURE, next frame as rendered)."""
    def make():
        from of_amd import synth
        g0, g1 = gray_pair(h, w, seed)
        return g0, synth.apply_exposure(g1, *EXPOSURE), g1
    return cached(("pair", h, w, seed), make)


def exposed(g):
    from of_amd import synth
    return synth.apply_exposure(g, *EXPOSURE)


# ---------------------------------------------------------------------------------------------------- 1. every window
def every_window_cases(windows=WINDOWS):
    """test_lk_every_window's frames and points with the next frame under EXPOSURE; per window and frame one call with flags 0 and
    one seeded (the points plus uniform noise of +-12 px) with the eigenvalue flag, both at max_level 3.  At max_level 3 the seed
    is 1.5 px off on the top level, so a third call runs the seed on level 0 alone, where a point that comes back from 9 px or
    more has left the LK_M = 8 pixel margin of the staged region on the way (restaged_rows), without the eigenvalue flag so that
    rule 6 runs behind it.  case.inner: the number of corner points at the end of the point set."""
    for win in windows:
        for h, w in LK_GEOMS + (LK_GEOMS_15 if win == 15 else ()):
            g0, g1, _ = exposed_pair(h, w, 1000 + h + w)
            inner = cached(("corners", h, w), lambda: corner_points(g0))
            pts = np.concatenate([border_points(h, w, win), inner])
            seed = pts + np.random.default_rng(100 * win + w).uniform(-12, 12, pts.shape).astype(np.float32)
            for flags, L in ((0, 3), (SEED_EIG, 3), (R.USE_INITIAL_FLOW, 0)):
                yield Case(f"win {win} {w}x{h} flags {flags} max_level {L} {light_kernel(win)}", g0, g1, pts, win, L, seed=seed if flags else None,
                           flags=flags, lk=dict(max_count=30, eps=0.01, min_eig_thr=1e-4), inner=len(inner), geom=(h, w))


def restaged_rows(case, nxt, st):
    """Tracked points of a level-0 seeded case that ended more than LK_M + 1 pixels from their seed along an axis: the integer
    window origin moved by more than LK_M, so k_lk_light restaged its next-frame region at least once."""
    assert case.L == 0 and case.flags & R.USE_INITIAL_FLOW
    return (np.asarray(st).ravel() == 1) & (np.abs(np.asarray(nxt).reshape(-1, 2) - case.seed[0]).max(axis=1) > pr.LK_M + 1)


# ---------------------------------------------------------------------------------------------------- 2. full contrast
FULL_WINDOWS = (3, 7, 11, 13, 15, 17, 21, 23, 31)
FULL_SHIFTS = ((0, 0), (1, -1), (0, 2))
FULL_DIVISORS = (1, 4)


def full_contrast_inputs():
    """The noise and "mixed" frames and the 40 integer-position + 24 quarter-pixel points of test_lk_full_contrast_every_kernel (the
    same generator in the same order), and the plaid.  -> (dict name -> frame, ipts [40,2], pts [64,2])."""
    def make():
        h, w = 120, 160
        rng = np.random.default_rng(9)
        noise = pr.binary_noise((h, w), 9)
        mixed = pr.stripes((h, w), flip_rows=9)
        mixed[:, w // 2:] = (rng.integers(0, 256, (h, w - w // 2)) // 4 + 96).astype(np.uint8)
        ipts = rng.integers([16, 16], [w - 16, h - 16], (40, 2)).astype(np.float32)
        fpts = (np.round(rng.uniform([-8, -8], [w + 8, h + 8], (24, 2)) * 4) / 4).astype(np.float32)
        return dict(noise=noise, plaid=pr.plaid((h, w)), mixed=mixed), ipts, np.concatenate([ipts, fpts])
    return cached("full", make)


def full_contrast_cases(windows=FULL_WINDOWS):
    """Per frame, brightness and window one batch of three: the next frames are the frame rolled by FULL_SHIFTS, divided by 1 or 4."""
    imgs, ipts, pts = full_contrast_inputs()
    for (name, img), div in itertools.product(imgs.items(), FULL_DIVISORS):
        g1 = np.stack([np.roll(img, s, axis=(0, 1)) // div for s in FULL_SHIFTS]).astype(np.uint8)
        for win in windows:
            yield Case(f"{name} / {div} win {win} {light_kernel(win)}", np.stack([img] * 3), g1, np.stack([pts] * 3), win, 2, name=name, div=div)


def row_sums(prev, nxt, ipts, win):
    """What the four 16-lane rows of sums_J (k_lk_light.inc, NPL <= 4) hold at the start position of integer-position points at
    level 0: there the bilinear weights are (2^14, 0, 0, 0), so jv = 32 J, and Ixp, Iyp are the Scharr derivatives of the previous
    frame (io.scharr).  Window pixel k = y win + x sits in lane k % 64, row lane / 16.
    -> (largest row sum of jv^2, largest |row sum| of jv ix, of jv iy) over the points, python ints."""
    assert win <= 15
    d = io.scharr(prev).astype(np.int64)
    J = nxt.astype(np.int64) * 32
    half = (win - 1) // 2
    row = (np.arange(win * win) % 64) // 16
    top = [0, 0, 0]
    for x, y in np.asarray(ipts).reshape(-1, 2):
        x, y = int(x), int(y)
        sl = (slice(y - half, y + half + 1), slice(x - half, x + half + 1))
        jv = J[sl].ravel(); ix = d[sl][..., 0].ravel(); iy = d[sl][..., 1].ravel()
        assert jv.size == win * win, (x, y, win)
        for i, prod in enumerate((jv * jv, jv * ix, jv * iy)):
            s = np.zeros(4, np.int64)
            np.add.at(s, row, prod)
            top[i] = max(top[i], int(np.abs(s).max()))
    return tuple(top)


# ---------------------------------------------------------------------------------------------------- 3. constant next frames
CONST_WINDOWS = (3, 9, 13, 15, 21, 31)
CONST_VALUES = (255, 0, 100)


def constant_cases():
    """A textured or a binary-noise previous frame against next frames that are all 255, all 0 and all 100 (one batch of three),
    the 64 points of the full-contrast section.  The mismatch vector is the template's half alone, so every step is the same drift;
    it is the longer the smaller the window, and a coarse level doubles it for every level below.  With three levels at windows 3
    and 9 fewer than 48 of the 64 points stay inside the frame (27 and 54 on the texture at windows 3 and 9), and on level 0 alone
    the large windows on noise move fewer than 16 points by a pixel (9 and 5 at windows 21 and 31): windows up to 9 run at
    max_level 0, the others at max_level 2."""
    h, w = 120, 160
    pts = full_contrast_inputs()[2]
    g1 = np.stack([np.full((h, w), v, np.uint8) for v in CONST_VALUES])
    for name, prev in (("textured", pr.textured(h, w, 31)), ("noise", pr.binary_noise((h, w), 9))):
        for win in CONST_WINDOWS:
            yield Case(f"{name} -> constant, win {win}", np.stack([prev] * 3), g1, np.stack([pts] * 3), win, 0 if win <= 9 else 2, name=name)


# ---------------------------------------------------------------------------------------------------- 4. clamp and gain_max range
GAIN_MAX = (1.0000001, 1.5, 4.0, 16.0, 1e3, 1e300)


def clamp_cases():
    """A pair sixteen times apart in gain, either way round: alpha wants 16 (next frame darker: the upper bound) or 1 / 16 (previous
    frame darker: the lower bound).  Window 15 on both, window 21 on both."""
    h, w = 120, 160
    t = pr.textured(h, w, 41)
    r = np.roll(t, (1, -1), axis=(0, 1))
    pts = full_contrast_inputs()[2]
    for win in (15, 21):
        yield Case(f"next-darker win {win}", t, r // 16, pts, win, 2)
        yield Case(f"prev-darker win {win}", t // 16, r, pts, win, 2)


# ---------------------------------------------------------------------------------------------------- 5. termination grid
def criteria_cases():
    """test_lk_termination_criteria_and_clamps' grid: full at window 15 on 120 x 160, thinned at windows 9, 19 and 27; the next frame
    under EXPOSURE.  -> (base case, [(max_count, eps, min_eig_thr)]); base.inner: the corner points lead the point set."""
    for (h, w), win, full in (((120, 160), 15, True), ((120, 160), 9, False), ((120, 160), 19, False), ((97, 131), 27, False)):
        g0, g1, _ = exposed_pair(h, w, 2000 + w + win)
        inner = corner_points(g0, 40)
        pts = np.concatenate([inner, border_points(h, w, win)[::5]])
        combos = list(itertools.product(CRIT_MAX_COUNT, CRIT_EPS, CRIT_MIN_EIG))
        if not full:
            combos = [(mc, e, CRIT_MIN_EIG[i % 3]) for i, (mc, e) in enumerate(itertools.product(CRIT_MAX_COUNT, CRIT_EPS))]
        seed = pts + np.random.default_rng(win).uniform(-3, 3, pts.shape).astype(np.float32)
        yield Case(f"{w}x{h} win {win}", g0, g1, pts, win, 3, seed=seed, inner=len(inner)), combos


def with_criteria(base, mc, eps, thr, flags=0):
    return Case(f"{base.tag} max_count {mc} eps {eps} min_eig {thr} flags {flags}", base.g0, base.g1, base.pts, base.win, base.L,
                seed=base.seed if flags & R.USE_INITIAL_FLOW else None, flags=flags, lk=dict(max_count=mc, eps=eps, min_eig_thr=thr))


# ---------------------------------------------------------------------------------------------------- 6. level cuts
def level_cut_cases(windows=(3, 15, 31)):
    """test_lk_level_cut's frames and points at max_level 8 with the next frame rolled by (1, -1) and under EXPOSURE.
    case.depth: the restated pyramid depth."""
    for win in windows:
        sizes = pr.cut_sizes(win)
        for h, w in sorted(set(zip(sizes, sizes[::-1])) | set(zip(sizes, sizes))):
            g0 = pr.textured(h, w, 40 + h + w)
            g1 = exposed(np.roll(g0, (1, -1), axis=(0, 1)))
            gx, gy = np.meshgrid(np.linspace(-2, w + 1, 7), np.linspace(-2, h + 1, 7))
            pts = np.concatenate([np.stack([gx.ravel(), gy.ravel()], 1), [[w / 2 + 0.25, h / 2 - 0.5]]]).astype(np.float32)
            depth = len(pr.lk_level_sizes(h, w, win, 8)) - 1
            yield Case(f"{w}x{h} win {win} levels {depth}", g0, g1, pts, win, 8, depth=depth, geom=(h, w))


# ---------------------------------------------------------------------------------------------------- 7. gates under the light
GATE_WINDOWS = (9, 15, 21)
GATE_COUNTS = (72, 41, 5)
GATE_ERR_MAX = 6.0
GATE_FB_THR = 0.5


def gate_scene(pkg, win):
    """Three 135 x 241 pairs under a yaw of 0.05 per frame (test_gpu_lk_seed.frames), the next frames under EXPOSURE, 72 points each
    (test_gpu_lk_seed.points).  -> g0, g1 [3,h,w], pts [3,72,2], counts."""
    def make():
        g0, g1, base = frames(pkg, 135, 241, 3)
        pts, _ = points(g0, base, 72, win, 700 + win)
        return g0, np.stack([exposed(a) for a in g1]), pts, np.array(GATE_COUNTS, np.int32)
    return cached(("gate", win), make)


def gate_settings():
    """fb "plain" and "seeded", fb_level -1 / 0 / 1, err_max off and on: track_gate_reference.setting dicts."""
    for fb, level, err_max in itertools.product(("plain", "seeded"), (-1, 0, 1), (0.0, GATE_ERR_MAX)):
        yield G.setting(fb=fb, fb_thr=GATE_FB_THR, fb_level=level, err_max=err_max)


def gated_reference(scene, win, L, gate, light):
    """lk_light_reference.gated per image over its own count -> [dict]."""
    g0, g1, pts, counts = scene
    return [LR.gated(g0[b], g1[b], pts[b, :c], win, L, gate=gate, light=light, **LK) for b, c in enumerate(counts)]


# ---------------------------------------------------------------------------------------------------- 8. far coordinates
FAR_POINT, FAR_SEEDS = 5, (11, 17)                              # rows of the far point and of the two far seeds


def far_cases(windows=(15, 21, 31)):
    """Corner points with a seed of a quarter pixel beside them; a point at (-1e6, 3), a seed of exactly (1e6, -1e6) and a seed of
    (999999.5, 20) among them: inside int, out of bounds at every level.  -> (case, the same case without the three)."""
    h, w = 120, 160
    g0, g1, _ = exposed_pair(h, w, 1000 + h + w)
    pts = cached(("corners", h, w), lambda: corner_points(g0)).copy()
    seed = pts + np.float32(0.25)
    fpts, fseed = pts.copy(), seed.copy()
    fpts[FAR_POINT] = (-1e6, 3.0)
    fseed[FAR_SEEDS[0]] = (1e6, -1e6)
    fseed[FAR_SEEDS[1]] = (999999.5, 20.0)
    for win in windows:
        yield (Case(f"far win {win}", g0, g1, fpts, win, 3, seed=fseed, flags=R.USE_INITIAL_FLOW),
               Case(f"near win {win}", g0, g1, pts, win, 3, seed=seed, flags=R.USE_INITIAL_FLOW))
