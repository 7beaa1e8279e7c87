"""GPU parity over the whole LK window range (odd 3..31) and the whole corner block-size range (1..45).

ofk_launch_lk (k_lk.hip) routes a window to k_lk15q, k_lk15, k_lk<21> or k_lk<31>; k_lk15 stages with dwords or bytes by level
geometry, owns one-pixel last segments at windows 5, 9 and 13, and reduces window sums past 2^31 on a branch of its own
(wave_sum_rows_scaled).  The corner launchers (k_corners.hip) route a block size to k_mineig_pair, k_mineig_stream or the LDS-tile
k_mineig<0, true> (candidates) and to k_mineig<3|7|12|0, false> (the map).  Every test compares with oracle/image_oracle.c bit for
bit (positions, err and responses as uint32; status and corners exactly) and asserts, with the routing restatements of
tests/param_ranges.py, that the kernels and paths it is about ran."""
import itertools

import numpy as np
import pytest

import param_ranges as pr
from oracle import image_oracle as io

pytestmark = pytest.mark.gpu

WINDOWS = tuple(range(3, 32, 2))
MOTION = dict(v=(0.004, -0.003, 0.002), omega=(0.004, -0.002, 0.006), d=1.0)


def lk_equal(ctx, prev, nxt, pts, what, **kw):
    gn, gs, ge = ctx.lk_pyr(prev, nxt, pts, **kw)
    rn, rs, re = io.lk_pyr(prev, nxt, pts, **kw)
    tag = (what, kw)
    assert np.array_equal(gs, rs), (tag, np.flatnonzero(gs.ravel() != rs.ravel())[:8])
    assert np.array_equal(gn.view(np.uint32), rn.view(np.uint32)), (tag, float(np.abs(gn - rn).max()))
    assert np.array_equal(ge.view(np.uint32), re.view(np.uint32)), tag
    return gn, gs.ravel(), ge


def border_points(h, w, win):
    """Points on and beyond every border, at integer, half- and quarter-pixel positions."""
    half = (win - 1) / 2
    xs = (-win - 1.5, -half - 0.25, -1.0, 0.0, 0.5, 3.25, w / 2 + 0.75, w - 4.5, w - 1.0, w + half - 0.5, w + win + 2.0)
    ys = (-win - 2.0, -half + 0.75, 0.0, 0.25, 2.5, h / 2 - 0.25, h - 3.75, h - 1.0, h + 0.5, h + half, h + win + 1.5)
    return np.array([[x, y] for x in xs for y in ys], np.float32)


def corner_points(g, n=48):
    """Shi-Tomasi corners of g, every second one moved to a half- or quarter-pixel position."""
    c = io.good_features(g, n, 0.01, 5, 5).reshape(-1, 2)
    off = np.array([[0, 0], [0.5, 0.5], [0, 0], [0.25, -0.75]], np.float32)
    return c + off[np.arange(len(c)) % 4]


def gray_pair(h, w, seed):
    from of_amd import synth
    p = synth.render_pair(h, w, seed, **MOTION)
    return io.gray_bgr8(p["prev"]), io.gray_bgr8(p["next"])


# ---------------------------------------------------------------------------------------------------- 1. every window
# a frame whose width is a multiple of 4 (dword prev staging), an odd-width frame (byte staging), and at win 15 a frame that takes
# k_lk15q and one where k_lk15q is refused at a coarse level (312 -> 156 -> 78) so that k_lk15 runs its dword next-frame staging
LK_GEOMS = ((120, 160), (97, 131))
LK_GEOMS_15 = ((256, 320), (256, 312))


def test_lk_every_window(gpu_ctx, pkg):
    pairs, seen, staging, frac = {}, set(), set(), {}
    for win in WINDOWS:
        tracked = []
        for h, w in LK_GEOMS + (LK_GEOMS_15 if win == 15 else ()):
            if (h, w) not in pairs:
                pairs[h, w] = gray_pair(h, w, 1000 + h + w)
            g0, g1 = pairs[h, w]
            inner = corner_points(g0)
            pts = np.concatenate([border_points(h, w, win), inner])
            kern = pr.lk_kernel(h, w, win, 3)
            seen.add(kern)
            if kern == "k_lk15":
                staging |= pr.lk15_staging(h, w, win, 3, pts)
            _, st, _ = lk_equal(gpu_ctx, g0, g1, pts, f"win {win} {w}x{h} {kern}", win=win, max_level=3, max_count=30, eps=0.01)
            tracked.append(st[-len(inner):])
        frac[win] = np.concatenate(tracked).mean()
    assert min(frac.values()) > 0.6, frac                  # real motion, tracked: the comparison is not one of lost points
    assert seen == pr.LK_KERNELS, seen
    assert staging == pr.LK15_STAGING, staging


# ---------------------------------------------------------------------------------------------------- 2. full contrast
def test_lk_full_contrast_every_kernel(gpu_ctx):
    """Binary noise, period-4 stripes (|Ix| = 4080), the diagonal checker and a half-stripes half-texture frame at windows whose
    integer sums pass 2^31: k_lk15 at 11 / 13 / 15 (the int64 branch of wave_sum_rows_scaled), k_lk<21> and k_lk<31> (wave_sum_i64).
    The sums of the integer-position points are restated in numpy from io.scharr."""
    h, w = 120, 160
    rng = np.random.default_rng(9)
    noise = pr.binary_noise((h, w), 9)
    mixed = pr.stripes((h, w), flip_rows=9)
    mixed[:, w // 2:] = (rng.integers(0, 256, (h, w - w // 2)) // 4 + 96).astype(np.uint8)      # one launch, both reduction paths
    imgs = dict(noise=noise, stripes=pr.stripes((h, w)), stripes_flipped=pr.stripes((h, w), flip_rows=9),
                hstripes=pr.stripes((h, w), axis=0), checker=pr.diagonal((h, w)), mixed=mixed)
    ipts = rng.integers([16, 16], [w - 16, h - 16], (40, 2)).astype(np.float32)
    fpts = (np.round(rng.uniform([-8, -8], [w + 8, h + 8], (24, 2)) * 4) / 4).astype(np.float32)
    pts = np.concatenate([ipts, fpts])
    seen, peak = set(), {}
    for win in (11, 13, 15, 17, 19, 21, 23, 27, 31):
        kern = pr.lk_kernel(h, w, win, 2)
        seen.add(kern)
        for name, img in imgs.items():
            s = pr.window_sums(img, ipts, win)
            peak[win] = max(peak.get(win, 0), int(s[:, [0, 2]].max()))
            for shift in ((0, 0), (1, -1), (0, 2)):
                lk_equal(gpu_ctx, img, np.roll(img, shift, axis=(0, 1)), pts, f"{name} win {win} {kern} shift {shift}",
                         win=win, max_level=2, max_count=20, eps=0.03)
    assert seen == {"k_lk15", "k_lk<21>", "k_lk<31>"}, seen
    assert all(peak[win] > pr.INT32_MAX for win in (13, 15, 17, 19, 21, 23, 27, 31)), peak
    m = pr.window_sums(mixed, ipts, 15)[:, 0]
    assert (m > pr.INT32_MAX).any() and (m < 2 ** 30).any()


# ---------------------------------------------------------------------------------------------------- 3. criteria, level cut, batch
CRIT_MAX_COUNT = (0, 1, 2, 100, 150)                      # 150: clamped to 100
CRIT_EPS = (0.0, 1e-12, 1e-7, 0.03, 10.0, 20.0)           # 20: clamped to 10
CRIT_MIN_EIG = (0.0, 1e-4, 1e-2)


def test_lk_termination_criteria_and_clamps(gpu_ctx, pkg):
    seen = set()
    for (h, w), win, full in (((256, 320), 15, True), ((120, 160), 9, True), ((120, 160), 19, False), ((97, 131), 27, False)):
        g0, g1 = gray_pair(h, w, 2000 + w + win)
        pts = np.concatenate([corner_points(g0, 40), border_points(h, w, win)[::5]])
        seen.add(pr.lk_kernel(h, w, win, 3))
        combos = list(itertools.product(CRIT_MAX_COUNT, CRIT_EPS, CRIT_MIN_EIG))
        if not full:
            combos = [(mc, e, CRIT_MIN_EIG[i % 3]) for i, (mc, e) in enumerate(itertools.product(CRIT_MAX_COUNT, CRIT_EPS))]
        res = {}
        for mc, eps, thr in combos:
            res[mc, eps, thr] = lk_equal(gpu_ctx, g0, g1, pts, f"{w}x{h} win {win}", win=win, max_level=3, max_count=mc, eps=eps,
                                         min_eig_thr=thr)
        for mc, eps, thr in combos:                           # the launcher's clamps: 150 runs as 100, eps 20 as 10
            for a, b in (((150, eps, thr), (100, eps, thr)), ((mc, 20.0, thr), (mc, 10.0, thr))):
                if a in res and b in res:
                    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(res[a], res[b])), (a, b)
    assert seen == pr.LK_KERNELS, seen


@pytest.fixture(scope="module")
def ctx16(ofk):
    """A small context of its own: batches up to 16 (the XCD remap needs batch % 8 == 0) and all nine pyramid levels."""
    c = ofk.Context(0, 320, 256, 16, 256, 8)
    yield c
    c.close()


def test_lk_level_cut(ctx16):
    """Frames whose (n + 1) / 2 chain lands on win (cut) or win + 1 (kept) one or two halvings down, at max_level 8."""
    for win in (3, 15, 31):
        sizes = pr.cut_sizes(win)
        depths = set()
        for h, w in sorted(set(zip(sizes, sizes[::-1])) | set(zip(sizes, sizes))):
            L = len(pr.lk_level_sizes(h, w, win, 8)) - 1
            assert io.lk_levels(h, w, win, 8) == L, (h, w, win)
            depths.add(L)
            g0 = pr.textured(h, w, 40 + h + w)
            g1 = np.roll(g0, (1, -1), axis=(0, 1))
            gx, gy = np.meshgrid(np.linspace(-2, w + 1, 7), np.linspace(-2, h + 1, 7))
            pts = np.concatenate([np.stack([gx.ravel(), gy.ravel()], 1), [[w / 2 + 0.25, h / 2 - 0.5]]]).astype(np.float32)
            lk_equal(ctx16, g0, g1, pts, f"{w}x{h} win {win} levels {L}", win=win, max_level=8, max_count=20, eps=0.03)
        assert len(depths) >= 2, (win, depths)


def test_lk_batch_xcd_remap(ctx16):
    """Batches of 8 and 16 (k_lk15 and k_lk15q remap blocks to XCDs when batch % 8 == 0) with ragged counts, 0 and 1 among them."""
    S = 96
    seen = set()
    for (h, w), win in (((256, 320), 15), ((256, 312), 15), ((120, 160), 7)):
        kern = pr.lk_kernel(h, w, win, 3)
        for B in (8, 16):
            imgs = [pr.textured(h, w, 300 + 17 * b + w) for b in range(B)]
            prev = np.stack(imgs)
            nxt = np.stack([np.roll(im, (1 + b % 3, -(b % 4)), axis=(0, 1)) for b, im in enumerate(imgs)])
            counts = np.array([(0, 1, S, 17, 2, S - 1, 33, 5)[(b + B // 8) % 8] for b in range(B)], np.int32)
            pts = np.zeros((B, S, 2), np.float32)
            for b in range(B):
                cand = np.concatenate([corner_points(prev[b], 64), border_points(h, w, win)])
                pts[b, :counts[b]] = cand[:counts[b]]
            gn, gs, ge = ctx16.lk_pyr(prev, nxt, pts, counts, win=win, max_level=3, max_count=20, eps=0.03)
            for b in range(B):
                n = int(counts[b])
                if n == 0:
                    continue
                rn, rs, re = io.lk_pyr(prev[b], nxt[b], pts[b, :n], win=win, max_level=3, max_count=20, eps=0.03)
                tag = (kern, B, b, n)
                assert np.array_equal(gs[b, :n], rs.ravel()), tag
                assert np.array_equal(gn[b, :n].view(np.uint32), rn.reshape(-1, 2).view(np.uint32)), tag
                assert np.array_equal(ge[b, :n].view(np.uint32), re.ravel().view(np.uint32)), tag
            seen.add((kern, B % 8 == 0))
    assert {k for k, remap in seen if remap} == {"k_lk15q", "k_lk15"}, seen


# ---------------------------------------------------------------------------------------------------- 4. every block size
def corner_mask(h, w, seed):
    rng = np.random.default_rng(seed)
    m = np.ones((h, w), np.uint8)
    m[:, : w // 3] = 0
    m[rng.integers(0, h, h // 4)] = 0
    return m


def test_corners_every_block_size(gpu_ctx, pkg):
    """ofk_mineig_response and ofk_good_features at every block size check_block accepts: the minimum image (bs + 4)^2, odd sizes
    that straddle the LDS-tile blocks, and for 3 / 5 / 7 the widths on both sides of the pair kernel's rule; noise and texture, a
    mask on every third image."""
    seen = set()
    for bs in range(1, 46):
        shapes = [(bs + 4, bs + 4), (bs + 4, bs + 4)] + pr.tile_edge_shapes(bs)
        if bs in (3, 5, 7):
            shapes += [(41, w) for w in (60, 64, 66, 68)]
        for i, (h, w) in enumerate(shapes):
            img = np.random.default_rng(bs * 100 + i).integers(0, 256, (h, w), dtype=np.uint8) if i % 2 == 0 else pr.textured(h, w, bs * 100 + i)
            mask = corner_mask(h, w, i) if i % 3 == 2 else None
            resp, cand = pr.corner_kernels(h, w, bs)
            tag = (bs, h, w, i, resp, cand)
            got = gpu_ctx.mineig(img, bs)
            assert np.array_equal(got.view(np.uint32), io.mineig(img, bs).view(np.uint32)), tag
            for mc, q, md in ((300, 0.01, 2.0), (20, 0.1, 6.0)):
                gp = gpu_ctx.good_features(img, mc, q, md, bs, mask=mask)
                rp = io.good_features(img, mc, q, md, bs, mask=mask)
                assert gp.shape == rp.shape and np.array_equal(gp, rp), (tag, mc, gp.shape, rp.shape)
            seen |= {resp, (bs, cand)}
    assert {s for s in seen if isinstance(s, str)} == {"k_mineig<3,false>", "k_mineig<7,false>", "k_mineig<12,false>", "k_mineig<0,false>"}
    cands = {s for s in seen if isinstance(s, tuple)}
    assert {(bs, "k_mineig_pair") for bs in (3, 5, 7)} | {(bs, "k_mineig_stream") for bs in (3, 5, 7, 12)} <= cands, cands
    assert {(bs, "k_mineig<0,true>") for bs in range(1, 46) if bs not in (3, 5, 7, 12)} <= cands, cands


# ---------------------------------------------------------------------------------------------------- 5. full-contrast blocks
FULL_BLOCKS = (2, 12, 25, 32, 40, 44, 45)


def test_corners_full_contrast_blocks(gpu_ctx):
    """Period-4 stripes (Sobel |dx| = 1020: Sxx = bs^2 1020^2, 98 % of 2^31 at 45 x 45), the diagonal pattern, binary noise and a
    plaid (stripes with a faint cross pattern, so that lambda_min is not zero where Sxx is at its largest) through the map and the
    corner kernels at large blocks.  The box sums are restated in int64."""
    h, w = 97, 131
    imgs = dict(vstripes=pr.stripes((h, w), 1), hstripes=pr.stripes((h, w), 0), diagonal=pr.diagonal((h, w)),
                noise=pr.binary_noise((h, w), 5), plaid=pr.plaid((h, w)))
    top = {}
    for bs in FULL_BLOCKS:
        for name, img in imgs.items():
            tag = (name, bs, pr.corner_kernels(h, w, bs))
            ref = io.mineig(img, bs)
            assert np.array_equal(gpu_ctx.mineig(img, bs).view(np.uint32), ref.view(np.uint32)), tag
            for mc, q, md in ((500, 0.001, 1.0), (50, 0.1, 5.0)):
                gp = gpu_ctx.good_features(img, mc, q, md, bs)
                rp = io.good_features(img, mc, q, md, bs)
                assert gp.shape == rp.shape and np.array_equal(gp, rp), (tag, mc, gp.shape, rp.shape)
            sxx, _, syy = pr.sobel_box_sums(img, bs)
            top[name, bs] = int(max(sxx.max(), syy.max()))
    assert top["vstripes", 45] == top["hstripes", 45] == 45 * 45 * 1020 ** 2 > 0.98 * 2 ** 31
    assert all(top[name, bs] > 2 ** 30 for name in ("vstripes", "hstripes", "plaid") for bs in (40, 44, 45)), top
    assert top["plaid", 45] > 0.8 * 2 ** 31 and np.max(io.mineig(imgs["plaid"], 45)) > 0


# ---------------------------------------------------------------------------------------------------- 7. randomised pipeline sweep
SWEEP_CASES, SWEEP_SEED = 150, 11


def test_pipeline_random_sweep(pkg, ofk):
    """tools/stress_parity.py's comparison at a bounded size: FlowPipeline against the oracle on random sizes (strip boundaries of
    the streaming kernels), block sizes 1..45, every odd window, corner budgets and pyramid depths.  A configuration the library
    refuses is a failure unless the oracle refuses it too."""
    cases = pr.sweep_cases(SWEEP_CASES, SWEEP_SEED)
    failures = [f for f in (pr.run_sweep_case(c, ofk) for c in cases) if f]
    assert not failures, failures[:10]
    assert {c["cfg"].win for c in cases} == set(WINDOWS)
    assert len({c["cfg"].block_size for c in cases}) >= 30
