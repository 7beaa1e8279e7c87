"""CPU-only: analytic known-answer tests and an independent numpy cross-check of oracle/image_oracle.c
(the image-stage oracle is parity-unpinned w.r.t. OpenCV; these pin it to SURVEY.md Appendix B)."""
import numpy as np
import pytest

from oracle import image_oracle as io


def r101(i, n):
    i = np.asarray(i)
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def np_conv_sep(img, kx, ky):
    """Separable correlation with REFLECT_101, integer."""
    h, w = img.shape
    rx, ry = len(kx) // 2, len(ky) // 2
    a = img.astype(np.int64)
    t = sum(kx[i] * a[:, r101(np.arange(w) + i - rx, w)] for i in range(len(kx)))
    return sum(ky[j] * t[r101(np.arange(h) + j - ry, h), :] for j in range(len(ky)))


@pytest.fixture(scope="module")
def img():
    return np.random.default_rng(0).integers(0, 256, (61, 83), dtype=np.uint8)


def test_gray_formula():
    bgr = np.random.default_rng(1).integers(0, 256, (17, 19, 3), dtype=np.uint8)
    b, g, r = [bgr[..., i].astype(np.int64) for i in range(3)]
    assert np.array_equal(io.gray_bgr8(bgr), ((b * 3735 + g * 19235 + r * 9798 + 16384) >> 15).astype(np.uint8))
    assert io.gray_bgr8(np.full((2, 2, 3), 255, np.uint8))[0, 0] == 255


def test_pyr_down_vs_numpy(img):
    full = np_conv_sep(img, [1, 4, 6, 4, 1], [1, 4, 6, 4, 1])
    assert np.array_equal(io.pyr_down(img), ((full[::2, ::2] + 128) >> 8).astype(np.uint8))
    assert io.pyr_down(img).shape == (31, 42)
    assert io.lk_levels(1080, 1920, 15, 3) == 3 and io.lk_levels(60, 60, 15, 5) == 1 and io.lk_levels(1080, 1920, 15, 8) == 6


def test_scharr_vs_numpy(img):
    d = io.scharr(img)
    assert np.array_equal(d[..., 0], np_conv_sep(img, [-1, 0, 1], [3, 10, 3]))
    assert np.array_equal(d[..., 1], np_conv_sep(img, [3, 10, 3], [-1, 0, 1]))


def np_mineig(img, bs):
    """Independent numpy restatement of the min-eigenvalue response (Sobel, box sums of the products, f32 formula)."""
    dx = np_conv_sep(img, [-1, 0, 1], [1, 2, 1]); dy = np_conv_sep(img, [1, 2, 1], [-1, 0, 1])
    h, w = img.shape
    an = bs // 2

    def box(p):
        t = sum(p[:, r101(np.arange(w) - an + i, w)] for i in range(bs))
        return sum(t[r101(np.arange(h) - an + j, h), :] for j in range(bs))

    sxx, sxy, syy = box(dx * dx), box(dx * dy), box(dy * dy)
    scale = 1.0 / (4.0 * bs * 255.0)
    kd, ko = np.float32(0.5 * scale * scale), np.float32(scale * scale)
    a = sxx.astype(np.float32) * kd; b = sxy.astype(np.float32) * ko; c = syy.astype(np.float32) * kd
    amc = a - c
    return ((a + c) - np.sqrt(amc * amc + b * b, dtype=np.float32)).astype(np.float32)


@pytest.mark.parametrize("bs", [3, 6, 7, 1, 2, 4, 12, 31, 45])
def test_mineig_vs_numpy(img, bs):
    assert np.array_equal(io.mineig(img, bs).view(np.uint32), np_mineig(img, bs).view(np.uint32))


@pytest.mark.parametrize("bs", [1, 2, 4, 12, 31, 45])
def test_mineig_vs_numpy_full_contrast_and_minimum_size(bs):
    """The GPU block-size sweep leans on the oracle at every block size: full-contrast patterns (period-4 stripes put Sxx at
    bs^2 * 1020^2, 98 % of 2^31 at 45 x 45, where the int32 box sums must still be exact) and the smallest image the library accepts."""
    from param_ranges import diagonal, plaid, sobel_box_sums, stripes
    rng = np.random.default_rng(bs)
    imgs = [stripes((61, 83)), stripes((61, 83), axis=0), plaid((61, 83)), diagonal((61, 83)),
            rng.integers(0, 256, (bs + 4, bs + 4), dtype=np.uint8), (rng.integers(0, 2, (bs + 4, bs + 5)) * 255).astype(np.uint8)]
    for k, im in enumerate(imgs):
        assert np.array_equal(io.mineig(im, bs).view(np.uint32), np_mineig(im, bs).view(np.uint32)), k
    sxx = sobel_box_sums(imgs[0], bs)[0]
    assert sxx.max() == bs * bs * 1020 ** 2 and np.array_equal(sxx, np_sobel_box(imgs[0], bs))


def np_sobel_box(img, bs):
    dx = np_conv_sep(img, [-1, 0, 1], [1, 2, 1])
    h, w = img.shape
    an = bs // 2
    t = sum((dx * dx)[:, r101(np.arange(w) - an + i, w)] for i in range(bs))
    return sum(t[r101(np.arange(h) - an + j, h), :] for j in range(bs))


def test_corner_kats():
    assert len(io.good_features(np.full((40, 40), 7, np.uint8), 10, 0.1, 3, 3)) == 0          # constant image
    sq = np.zeros((120, 160), np.uint8); sq[40:80, 50:110] = 255
    pts = io.good_features(sq, 10, 0.5, 10, 3).reshape(-1, 2)
    assert len(pts) == 4
    for cx, cy in [(50, 40), (109, 40), (50, 79), (109, 79)]:
        assert np.min(np.hypot(pts[:, 0] - cx, pts[:, 1] - cy)) <= 1.5
    # translation equivariance away from the border
    rng = np.random.default_rng(3)
    base = rng.integers(0, 256, (140, 180), dtype=np.uint8)
    a = io.good_features(base[10:110, 10:150], 30, 0.2, 8, 5).reshape(-1, 2)
    eig_a = io.mineig(base[10:110, 10:150], 5); eig_b = io.mineig(base[15:115, 17:157], 5)
    assert np.array_equal(eig_a[15:80, 17:120], eig_b[10:75, 10:113])
    assert len(a) > 5
    # min-distance respected, ordering by response
    eig = io.mineig(base, 5)
    p, _ = io.select_corners(eig, 50, 0.05, 9.0)
    p = p.reshape(-1, 2)
    dist = np.hypot(p[:, None, 0] - p[None, :, 0], p[:, None, 1] - p[None, :, 1]) + 1e9 * np.eye(len(p))
    assert dist.min() >= 9.0
    vals = eig[p[:, 1].astype(int), p[:, 0].astype(int)]
    assert np.all(np.diff(vals) <= 0)
    # mask
    m = np.ones_like(base); m[:, :90] = 0
    pm = io.good_features(base, 20, 0.1, 5, 5, mask=m).reshape(-1, 2)
    assert len(pm) and np.all(pm[:, 0] >= 90)


def test_lk_kats():
    rng = np.random.default_rng(5)
    t = rng.standard_normal((200, 260))
    k = np.exp(-0.5 * (np.arange(-6, 7) / 2.0) ** 2); k /= k.sum()
    t = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 1, t); t = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 0, t)
    img = np.clip(127 + 60 * t / t.std(), 0, 255).astype(np.uint8)
    pts = io.good_features(img, 40, 0.05, 12, 7)
    # identical frames: zero displacement, status 1, err 0
    n, s, e = io.lk_pyr(img, img, pts)
    assert np.all(s == 1) and np.array_equal(n, pts) and np.all(e == 0)
    # integer translation of a smooth texture
    sh = np.roll(img, (3, -2), axis=(0, 1))
    n, s, e = io.lk_pyr(img, sh, pts)
    p2 = pts.reshape(-1, 2)
    inner = (p2[:, 0] > 30) & (p2[:, 0] < 230) & (p2[:, 1] > 30) & (p2[:, 1] < 170) & (s.ravel() == 1)
    assert inner.sum() > 10 and np.allclose((n.reshape(-1, 2) - p2)[inner], [-2, 3], atol=0.02)
    # window leaves the padded image -> status 0; flat patch -> rejected
    far = np.array([[-40.0, 10.0], [400.0, 50.0]], np.float32)
    n, s, e = io.lk_pyr(img, sh, far)
    assert np.all(s == 0) and np.all(e == 0)
    flat = np.full_like(img, 90)
    n, s, e = io.lk_pyr(flat, flat, pts)
    assert np.all(s == 0)


@pytest.fixture(scope="module")
def smooth():
    rng = np.random.default_rng(5)
    t = rng.standard_normal((200, 260))
    k = np.exp(-0.5 * (np.arange(-6, 7) / 2.0) ** 2); k /= k.sum()
    t = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 1, t); t = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 0, t)
    return np.clip(127 + 60 * t / t.std(), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("win", range(3, 32, 2))
def test_lk_kats_every_window(smooth, win):
    """Known answers at every window the library accepts: identical frames give zero flow, status 1, err 0; an integer translation
    of a smooth texture is recovered."""
    pts = io.good_features(smooth, 40, 0.05, 12, 7)
    n, s, e = io.lk_pyr(smooth, smooth, pts, win=win)
    assert np.all(s == 1) and np.array_equal(n, pts) and np.all(e == 0)
    n, s, e = io.lk_pyr(smooth, np.roll(smooth, (3, -2), axis=(0, 1)), pts, win=win)
    p2 = pts.reshape(-1, 2)
    inner = (p2[:, 0] > 40) & (p2[:, 0] < 220) & (p2[:, 1] > 40) & (p2[:, 1] < 160) & (s.ravel() == 1)
    dev = np.abs((n.reshape(-1, 2) - p2)[inner] - [-2, 3])
    hit = (dev < 0.05).all(1).mean()                          # a 3 x 3 window can lock onto a wrong match of a smooth texture
    assert inner.sum() > 8 and np.median(dev) < 0.02 and hit >= (0.7 if win == 3 else 1.0), (win, np.median(dev), hit)


def test_lk_levels_at_the_cut():
    """io.lk_levels against the level rule restated (tests/param_ranges.py), on sides where a level lands on win or win + 1."""
    from param_ranges import cut_sizes, lk_level_sizes
    for win in range(3, 32, 2):
        sizes = cut_sizes(win) + [1000]
        for h in sizes:
            for w in sizes:
                for ml in (0, 1, 2, 3, 8):
                    assert io.lk_levels(h, w, win, ml) == len(lk_level_sizes(h, w, win, ml)) - 1, (h, w, win, ml)
    assert io.lk_levels(29, 1000, 15, 8) == 0 and io.lk_levels(31, 1000, 15, 8) == 1 and io.lk_levels(64, 1000, 15, 8) == 2
    assert io.lk_levels(5, 6, 3, 8) == 0 and io.lk_levels(8, 8, 3, 8) == 1 and io.lk_levels(16, 16, 3, 8) == 2
