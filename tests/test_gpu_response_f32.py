"""GPU parity of the response kernel's two datapaths (k_corners.hip, k_mineig_pair): the f32 rows are exact while every window's
Sxx + Syy stays within 2^24, and a strip whose sums reach it is restarted on the integer rows.  Images on both sides of the bound,
and frames where both paths run in one launch, must give the oracle's corners bit for bit."""
import numpy as np
import pytest

from oracle import image_oracle as io

pytestmark = pytest.mark.gpu

TWO24 = 1 << 24


def max_window_sum(img, bs):
    """max over pixels of Sxx + Syy of the bs x bs window (Sobel 3x3, reflect-101 borders), in exact integers."""
    g = np.pad(img.astype(np.int64), 1, mode="reflect")
    s = g[:-2] + 2 * g[1:-1] + g[2:]
    dx = s[:, 2:] - s[:, :-2]
    t = g[2:] - g[:-2]
    dy = t[:, :-2] + 2 * t[:, 1:-1] + t[:, 2:]
    p = np.pad(dx * dx + dy * dy, bs // 2, mode="reflect")
    c = np.cumsum(np.cumsum(np.pad(p, ((1, 0), (1, 0))), 0), 1)
    box = c[bs:, bs:] - c[:-bs, bs:] - c[bs:, :-bs] + c[:-bs, :-bs]
    return int(box.max())


def corners_equal(gpu_ctx, img, mc, q, md, bs, mask=None):
    got = gpu_ctx.good_features(img, mc, q, md, bs, mask=mask)
    ref = io.good_features(img, mc, q, md, bs, mask=mask)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(got, ref)
    return got


def stripes(h, w, amp, vertical=True, base=40):
    x = np.arange(w if vertical else h)
    row = np.where((x % 4) >= 2, amp, 0) + base
    img = np.broadcast_to(row[None, :], (h, w)) if vertical else np.broadcast_to(row[:, None], (h, w))
    return np.ascontiguousarray(img).astype(np.uint8)


def checker(h, w, amp, base=40):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy // 2) + (xx // 2)) % 2) * amp + base).astype(np.uint8)


def with_blobs(img, seed, level):
    """A few flat squares of one grey level on top, so that there are corners to pick besides the periodic pattern."""
    rng = np.random.default_rng(seed)
    out = img.copy()
    for _ in range(12):
        y, x = rng.integers(8, img.shape[0] - 24), rng.integers(8, img.shape[1] - 24)
        out[y:y + 12, x:x + 12] = level
    return out


@pytest.mark.parametrize("amp", [146, 147])
@pytest.mark.parametrize("shape", [(240, 320), (200, 644), (135, 1000)])
def test_period4_stripes_at_the_bound(gpu_ctx, amp, shape):
    """Period-4 stripes: |dx| = 4 amp everywhere, so a 7x7 window holds 784 amp^2 - 16.71 M for 146 (f32 rows), 16.94 M for 147
    (above 2^24: the integer rows).  Widths 320 / 644 / 1000 give one, six and nine strips with mirrored border columns."""
    h, w = shape
    for vertical in (True, False):
        img = with_blobs(stripes(h, w, amp, vertical), amp + w, 40 + amp // 2)
        assert (max_window_sum(img, 7) >= TWO24) == (amp == 147)
        for bs in (7, 5, 3):
            corners_equal(gpu_ctx, img, 300, 0.01, 4, bs)


@pytest.mark.parametrize("amp", [146, 255])
def test_checkerboard_patches(gpu_ctx, amp):
    """2 x 2-cell checkerboard patches on a faint background (a whole frame of them ties everywhere and overflows the candidate
    list): 255 puts the patch windows above 2^24, 146 keeps them below."""
    rng = np.random.default_rng(amp)
    h, w = 256, 384
    img = rng.integers(100, 112, (h, w)).astype(np.uint8)
    img[60:68, 40:300] = checker(8, 260, amp, base=0)
    assert (max_window_sum(img, 7) >= TWO24) == (amp == 255)
    for bs in (7, 5, 3):
        corners_equal(gpu_ctx, img, 400, 0.01, 3, bs)
        corners_equal(gpu_ctx, img, 50, 0.3, 10, bs)


def noisy_strips_1080p(seed):
    """A textured 1080p frame with full-contrast 0/255 noise in a few column bands and row bands only: windows there pass 2^24 (the
    strips that touch them restart on the integer rows), the rest of the frame stays on the f32 rows - both in one launch."""
    from of_amd import synth
    rng = np.random.default_rng(seed)
    img = np.clip(np.rint(synth.make_texture(1080, 1920, seed)), 0, 255).astype(np.uint8)
    for x0 in (0, 700, 1850):
        img[:, x0:x0 + 40] = rng.integers(0, 2, (1080, min(40, 1920 - x0))) * 255
    img[500:530, 1000:1300] = rng.integers(0, 2, (30, 300)) * 255
    return img


def test_1080p_noise_bands_both_paths_in_one_launch(gpu_ctx, pkg):
    img = noisy_strips_1080p(21)
    assert max_window_sum(img, 7) >= TWO24
    assert max_window_sum(img[:, 100:600], 7) < TWO24 - 256
    for mc, q, md, bs in ((500, 0.01, 10, 7), (2000, 0.001, 3, 7), (1000, 0.005, 5, 5), (1000, 0.005, 5, 3)):
        corners_equal(gpu_ctx, img, mc, q, md, bs)


def test_1080p_noise_bands_with_mask(gpu_ctx, pkg):
    """The mask path (k_mineig_pair<BS, true>): the maximum and the keys of the masked-out noise bands must not count."""
    img = noisy_strips_1080p(22)
    mask = np.ones(img.shape, np.uint8)
    mask[:, 650:800] = 0
    mask[400:600, :] = 0
    for bs in (7, 5, 3):
        pts = corners_equal(gpu_ctx, img, 500, 0.01, 8, bs, mask=mask)
        assert len(pts) > 0


@pytest.mark.parametrize("bs", [7, 5, 3])
def test_full_contrast_plateau_rows_fill_the_key_buffer(gpu_ctx, bs):
    """A 0/255 tile whose period equals the box size: plateau rows of identical responses (a key per column, spills in front of every
    second row) at sums near or above 2^24 - spilled keys of a strip that restarts are overwritten by the integer pass."""
    rng = np.random.default_rng(30 + bs)
    h, w = 216, 640
    img = rng.integers(100, 112, (h, w)).astype(np.uint8)
    tile = (rng.integers(0, 2, (bs, bs)) * 255).astype(np.uint8)
    ph, pw = 6 + 2 * (bs // 2 + 1) + 1, 300
    img[40:40 + ph, 100:100 + pw] = np.tile(tile, (ph // bs + 1, pw // bs + 1))[:ph, :pw]
    for mc, q, md in ((300, 0.001, 0.0), (500, 0.01, 3.0)):
        corners_equal(gpu_ctx, img, mc, q, md, bs)


def test_pipeline_corners_on_both_paths(pkg):
    """The resident pipeline's corners (batch of two 1080p pairs: one ordinary texture, one with noise bands) equal the oracle's."""
    import of_amd.ofk as ofk
    from of_amd import synth
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    cfg = PipelineConfig(max_corners=500, quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)
    h, w = 1080, 1920
    pair = synth.render_pair(h, w, seed=5, v=(0.004, -0.003, 0.002), omega=(0.003, -0.002, 0.004), d=1.0)
    g_noise = noisy_strips_1080p(23)
    bgr_noise = np.repeat(g_noise[:, :, None], 3, axis=2)
    prev = np.stack([pair["prev"], bgr_noise])
    nxt = np.stack([pair["next"], bgr_noise])
    pipe = FlowPipeline(w, h, batch=2, cfg=cfg, device=0)
    sensors = ofk.make_sensors(2, d=pair["d"], normal=pair["n"], omega=pair["omega"], scaling=pair["scaling"], cx=pair["cx"], cy=pair["cy"])
    pipe.upload(prev, nxt, sensors)
    out = pipe.run()
    for b in range(2):
        g0 = io.gray_bgr8(prev[b])
        ref = io.good_features(g0, cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size)
        n = int(out["counts"][b])
        assert n == len(ref)
        assert np.array_equal(out["prev_pts"][b, :n], ref.reshape(-1, 2))
