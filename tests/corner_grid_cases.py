"""The cases the corner-grid GPU tests run (tests/test_gpu_corner_grid.py) and the CPU companion checks for non-vacuity
(tests/test_corner_grid_cases.py): scenes, settings, occupancy lists and the reference's answers, computed once per process.
Scenes are band-limited noise with one high-contrast box, the case an uncapped selection spends its whole budget on.
Test infrastructure only."""
import numpy as np

from oracle import image_oracle as io
import corner_grid_reference as R

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def band_noise(h, w, sigma, seed, box=None, amp=(12.0, 55.0)):
    """Gaussian low-passed white noise (sigma in cycles / px) at amplitude amp[0] around 128, amp[1] inside box = (y0, x0, bh, bw)."""
    rng = np.random.default_rng(seed)
    f = np.fft.fft2(rng.standard_normal((h, w)))
    fy, fx = np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :]
    n = np.real(np.fft.ifft2(f * np.exp(-(fx ** 2 + fy ** 2) / (2 * sigma ** 2))))
    n /= n.std()
    a = np.full((h, w), float(amp[0]))
    if box:
        y0, x0, bh, bw = box
        a[y0:y0 + bh, x0:x0 + bw] = amp[1]
    return np.clip(128 + a * n, 0, 255).astype(np.uint8)


QUALITY_SCENE = dict(h=480, w=640, sigma=0.08, seed=2, box=(120, 200, 200, 230), max_corners=300, quality=0.01, min_distance=10, block=7,
                     grid=(64, 4, 0))


def scene(name):
    def make():
        if name == "a":                                          # 240 x 320 (rows x columns), 8 x 6 cells of 40
            return band_noise(240, 320, 0.12, 11, box=(60, 100, 80, 80))
        if name == "b":                                          # ragged last row and column of cells of 37, pitch no multiple of 4
            return band_noise(243, 317, 0.12, 12, box=(100, 60, 80, 80))
        if name == "tiny":                                       # 32 x 64: cell 1 makes OFK_GRID_MAX_CELLS cells
            return band_noise(32, 64, 0.2, 13)
        if name == "big":                                        # more than 1024 corners wanted: the 1024-thread kernel
            return band_noise(480, 640, 0.12, 14, box=(200, 300, 80, 80))
        if name == "quality":
            q = QUALITY_SCENE
            return band_noise(q["h"], q["w"], q["sigma"], q["seed"], box=q["box"])
        raise KeyError(name)
    return cached(("scene", name), make)


def eig_of(name, block):
    return cached(("eig", name, block), lambda: io.mineig(scene(name), block))


def plateau_map():
    """A response map of few distinct values for ofk_select_corners_grid: a lattice of equal peaks (all tied, ranked by index alone),
    two flat plateaus whose every pixel is a 3x3 maximum, and a handful of higher singles."""
    def make():
        e = np.zeros((96, 128), np.float32)
        e[2:94:3, 2:126:3] = 1.0
        e[20:36, 40:72] = 2.0
        e[60:70, 8:30] = 2.0
        e[50, 100] = e[10, 10] = e[80, 64] = 3.0
        return e
    return cached("plateau", make)


def _occ_lists():
    """Three images' occupancy lists for scene "a", cell 40, cap 2 (rows of 100 points): some cells closed (and points outside the
    image, a NaN and points beyond the count mixed in), every cell closed, none listed."""
    S = 100
    pts = np.zeros((3, S, 2), np.float32); counts = np.zeros(3, np.int32)
    some = [(45.5, 45.9), (50.0, 70.0), (130.2, 90.7), (140.0, 100.0), (159.9, 119.9), (125.0, 85.0), (300.0, 10.0), (-3.0, 20.0), (10.0, 240.0),
            (320.0, 5.0), (np.nan, 50.0), (-0.5, 0.5), (0.2, -0.7), (279.0, 239.0)]
    pts[0, :len(some)] = some; counts[0] = len(some)
    pts[0, len(some):len(some) + 6] = [(20, 20), (21, 21), (60, 20), (61, 21), (100, 20), (101, 21)]   # beyond the count: ignored
    full = [(40 * cx + 7 + k, 40 * cy + 9 + k) for cy in range(6) for cx in range(8) for k in range(2)]
    pts[1, :len(full)] = full; counts[1] = len(full)
    return pts, counts


def _case(id, scene_name, max_corners, min_distance, grid, block=3, quality=0.01, mask=None, occ=None, designated=()):
    """designated: the non-vacuity conditions the companion asserts: "binds" (differs from plain), "deep" (examined > 512), "full"
    (every cell full, under budget), "inround" (more than cap candidates of one cell in an aligned run of 64), "plain" (equals plain)."""
    return dict(id=id, scene=scene_name, max_corners=max_corners, min_distance=min_distance, grid=grid, block=block, quality=quality,
                mask=mask, occ=occ, designated=tuple(designated))


def _mask_a():
    m = np.ones((1, 240, 320), np.uint8)
    m[:, 60:140, 100:180] = 0                                    # the box itself is masked out
    m[:, :, :25] = 0
    return m


CASES = [
    _case("a-cap1-md3", "a", 64, 3, (40, 1, 0), designated=("binds", "deep", "full")),
    _case("a-cap1-md0", "a", 64, 0, (40, 1, 0), designated=("binds", "deep", "full")),
    _case("a-cap2-md3", "a", 64, 3, (40, 2, 0), designated=("binds", "inround")),
    _case("a-cap2-md0", "a", 64, 0, (40, 2, 0), designated=("binds", "inround")),
    _case("a-cap3-md3", "a", 64, 3, (40, 3, 0), designated=("binds", "inround")),
    _case("a-cap255", "a", 64, 3, (40, 255, 0), designated=("plain",)),
    _case("b-cap1", "b", 100, 5, (37, 1, 0), designated=("binds", "deep", "full")),
    _case("b-cap2", "b", 100, 5, (37, 2, 0), designated=("binds",)),
    _case("a-one-cell", "a", 64, 3, (320, 10, 0), designated=("binds", "full")),
    _case("tiny-cell1", "tiny", 2000, 0, (1, 1, 0), designated=("plain",)),
    _case("tiny-cell1-md2", "tiny", 2000, 2, (1, 1, 0), designated=("plain",)),
    _case("a-occupancy", "a", 64, 3, (40, 2, 0), occ=_occ_lists(), designated=("binds",)),
    _case("a-mask", "a", 64, 3, (40, 2, 0), mask=_mask_a(), designated=("binds",)),
    _case("a-rank100", "a", 64, 3, (40, 1, 100), designated=("binds",)),
    _case("a-rank512", "a", 64, 3, (40, 1, 512), designated=("binds",)),
    _case("a-rank560", "a", 64, 3, (40, 1, 560), designated=("binds", "deep")),
    _case("a-rank-loose", "a", 64, 3, (40, 1, 100000), designated=("binds", "deep", "full")),
    _case("big-1200", "big", 1200, 3, (32, 3, 0), designated=("binds", "deep")),
]
PLATEAU_CASES = [
    dict(id="plateau-cap3", max_corners=200, quality=0.01, min_distance=2, grid=(16, 3, 0)),
    dict(id="plateau-cap1-md0", max_corners=200, quality=0.01, min_distance=0, grid=(16, 1, 0)),
    dict(id="plateau-rank", max_corners=200, quality=0.01, min_distance=2, grid=(16, 3, 300)),
]


def images(case):
    """gray [B,h,w] of a case: the occupancy case is a batch of three copies of its scene (the lists differ), all others one image."""
    g = scene(case["scene"])
    return np.stack([g] * (3 if case["occ"] is not None else 1))


def reference(case, plain=False):
    """Per image (points, (accepted, examined), ranks) of the reference; plain: the same call with the grid off."""
    def make():
        e = eig_of(case["scene"], case["block"])
        out = []
        for b in range(len(images(case))):
            m = None if case["mask"] is None else case["mask"][b]
            o = None if case["occ"] is None or plain else case["occ"][0][b, :case["occ"][1][b]]
            out.append(R.select(e, case["max_corners"], case["quality"], case["min_distance"], m, R.OFF if plain else case["grid"], o))
        return out
    return cached(("ref", case["id"], plain), make)


def plateau_reference(case, plain=False):
    return cached(("pref", case["id"], plain), lambda: R.select(plateau_map(), case["max_corners"], case["quality"], case["min_distance"],
                                                                 None, R.OFF if plain else case["grid"]))
