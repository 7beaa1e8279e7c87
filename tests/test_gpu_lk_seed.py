"""GPU: ofk_lk_pyr_ex (OFK_LK_USE_INITIAL_FLOW, OFK_LK_GET_MIN_EIGENVALS) and ofk_predict_points against the test-side reference
(tests/lk_seed_reference.py), bit-exact, on every kernel route: k_lk15q (window 15, quad-eligible levels), k_lk15 (window 15 on
other sizes, windows 3-13), k_lk<21> (17-21), k_lk<31> (23-31)."""
import numpy as np
import pytest

from oracle import image_oracle as io
import lk_seed_reference as R  # noqa: E402  (tests/lk_seed_reference.py)

pytestmark = pytest.mark.gpu

_frames = {}


def frames(pkg, h, w, batch):
    """`batch` gray frame pairs under a yaw of 0.05 per frame (flows up to ~20 px at 640 x 480) and their homographies."""
    key = (h, w, batch)
    if key not in _frames:
        from of_amd import synth
        prev, nxt, base = synth.make_batch(batch, h, w, 40, distinct=min(batch, 2), v=(0.004, -0.003, 0.001), omega=(0.002, -0.001, 0.05),
                                           margin=64)
        g0 = np.stack([io.gray_bgr8(a) for a in prev]); g1 = np.stack([io.gray_bgr8(a) for a in nxt])
        _frames[key] = (g0, g1, base)
    return _frames[key]


def points(g0, base, S, win, seed):
    """[B,S,2] points: corners, uniformly random positions and a frame of border points; `truth` = where the pair's motion takes them."""
    from of_amd import synth
    B, h, w = g0.shape
    rng = np.random.default_rng(seed)
    pts = np.zeros((B, S, 2), np.float32); truth = np.zeros((B, S, 2), np.float32)
    edge = np.array([(-2.5, 9.0), (0.3, 0.2), (w - 1.2, 4.5), (w + 1.0, h / 2), (w / 2, -1.5), (w / 2, 0.4), (w / 2, h - 0.6), (w / 3, h + 2.0),
                     (1.5, h - 1.5), (w - 1.5, h - 1.5), (w - 0.5, 0.5), (win / 2.0, win / 2.0)], np.float32)
    for b in range(B):
        c = io.good_features(g0[b], S // 2, 0.01, 5, 5).reshape(-1, 2)
        r = np.stack([rng.uniform(0, w, S), rng.uniform(0, h, S)], 1).astype(np.float32)
        p = np.concatenate([edge, c, r])[:S]
        pts[b] = p
        truth[b] = (p.astype(np.float64) + synth.true_flow_px(base[b % len(base)]["H"], p)).astype(np.float32)
    return pts, truth


def seed_kinds(pts, truth, h, w, seed):
    rng = np.random.default_rng(seed)
    noise = rng.uniform(-40, 40, pts.shape).astype(np.float32)
    outside = truth.copy()
    outside[:, 0::4] = (-300.0, -200.0); outside[:, 1::4, 0] += w + 100.0; outside[:, 2::4, 1] -= h + 50.0; outside[:, 3::4] = (9.9e5, -9.9e5)
    return (("truth", truth), ("noisy", truth + noise), ("outside", outside), ("points", pts.copy()))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def check(ctx, g0, g1, pts, counts, win, L, seed, flags, tag, lk=None):
    lk = lk or dict(max_count=20, eps=0.03, min_eig_thr=1e-4)
    got = ctx.lk_pyr(g0, g1, pts, counts, win=win, max_level=L, next_pts=seed, flags=flags, **lk)
    for b in range(len(g0)):
        n = int(counts[b])
        ref = R.lk_pyr(g0[b], g1[b], pts[b, :n], win, L, seed=None if seed is None else seed[b, :n], flags=flags, **lk)
        for name, g, r in zip(("next", "status", "err"), got, ref):
            g = g[b, :n]; r = r.reshape(g.shape)
            assert np.array_equal(bits(g), bits(r)), (tag, "image", b, name, int(np.sum(bits(g) != bits(r))), "of", g.size)
    return got


# (h, w), window, max_level: the route each case takes is named in its id
ROUTES = [
    pytest.param((480, 640), 15, 0, id="lk15q-L0"), pytest.param((480, 640), 15, 1, id="lk15q-L1"),
    pytest.param((480, 640), 15, 2, id="lk15q-L2"), pytest.param((480, 640), 15, 3, id="lk15q-L3"),
    pytest.param((240, 320), 15, 3, id="lk15-w15-level3-too-small-for-quad"), pytest.param((135, 241), 15, 2, id="lk15-w15-odd-size"),
    pytest.param((480, 640), 3, 2, id="lk15-w3"), pytest.param((480, 640), 7, 3, id="lk15-w7"), pytest.param((135, 241), 13, 1, id="lk15-w13"),
    pytest.param((480, 640), 17, 3, id="lk21-w17"), pytest.param((135, 241), 19, 2, id="lk21-w19"), pytest.param((480, 640), 21, 0, id="lk21-w21-L0"),
    pytest.param((480, 640), 23, 2, id="lk31-w23"), pytest.param((135, 241), 31, 1, id="lk31-w31"), pytest.param((480, 640), 31, 3, id="lk31-w31-L3"),
    pytest.param((40, 56), 15, 3, id="level-cut-w15"), pytest.param((70, 90), 31, 3, id="level-cut-w31"),
]


@pytest.mark.parametrize("shape,win,L", ROUTES)
def test_lk_pyr_ex_matches_reference(pkg, gpu_ctx, shape, win, L):
    h, w = shape
    B, S = 3, 72
    g0, g1, base = frames(pkg, h, w, B)
    pts, truth = points(g0, base, S, win, 100 + win)
    counts = np.array([S, 41, 5], np.int32)                    # ragged
    if min(h, w) < 100:
        assert io.lk_levels(h, w, win, L) < L                  # the winSize rule cuts the pyramid here
    plain = check(gpu_ctx, g0, g1, pts, counts, win, L, None, 0, "plain")
    eig = check(gpu_ctx, g0, g1, pts, counts, win, L, None, R.GET_MIN_EIGENVALS, "eig")
    for b in range(B):
        n = counts[b]
        assert np.array_equal(bits(eig[0][b, :n]), bits(plain[0][b, :n])) and np.array_equal(eig[1][b, :n], plain[1][b, :n])
    for kind, seed in seed_kinds(pts, truth, h, w, 7 * win + L):
        s4 = check(gpu_ctx, g0, g1, pts, counts, win, L, seed, R.USE_INITIAL_FLOW, kind + "/seed")
        s12 = check(gpu_ctx, g0, g1, pts, counts, win, L, seed, R.USE_INITIAL_FLOW | R.GET_MIN_EIGENVALS, kind + "/seed+eig")
        for b in range(B):
            n = counts[b]
            assert np.array_equal(bits(s12[0][b, :n]), bits(s4[0][b, :n])) and np.array_equal(s12[1][b, :n], s4[1][b, :n])
            if kind == "points":                               # a seed equal to the points is the plain call
                for g, p in zip(s4, plain):
                    assert np.array_equal(bits(g[b, :n]), bits(p[b, :n]))


def test_seeding_helps_where_the_plain_search_fails(pkg, gpu_ctx):
    """Not a parity statement: the seeds of this file do change the outcome (the comparison above is not vacuous)."""
    g0, g1, base = frames(pkg, 480, 640, 3)
    pts, truth = points(g0, base, 72, 15, 115)
    counts = np.array([72, 72, 72], np.int32)
    plain = gpu_ctx.lk_pyr(g0, g1, pts, counts, win=15, max_level=0)
    seeded = gpu_ctx.lk_pyr(g0, g1, pts, counts, win=15, max_level=0, next_pts=truth, flags=R.USE_INITIAL_FLOW)
    far = np.linalg.norm(truth[0] - pts[0], axis=1) > 8
    ok = lambda r: (r[1][0] == 1) & (np.linalg.norm(r[0][0] - truth[0], axis=1) < 0.5)
    assert ok(seeded)[far].sum() > 2 * ok(plain)[far].sum() + 5


@pytest.mark.parametrize("win,L", [(15, 3), (15, 0), (9, 2), (21, 2)])
def test_batch_of_eight_ragged(pkg, ofk, win, L):
    """A multiple of 8 images takes the XCD-aware block map of k_lk15q / k_lk15; counts from 0 to the stride."""
    h, w, B, S = 480, 640, 8, 64
    g0, g1, base = frames(pkg, h, w, B)
    pts, truth = points(g0, base, S, win, 300 + win)
    counts = np.array([S, 0, 1, 63, 4, 5, 33, 17], np.int32)
    ctx = ofk.Context(0, w, h, B, S, 3)
    try:
        check(ctx, g0, g1, pts, counts, win, L, None, 0, "plain")
        for kind, seed in seed_kinds(pts, truth, h, w, 11)[:2]:
            check(ctx, g0, g1, pts, counts, win, L, seed, R.USE_INITIAL_FLOW | R.GET_MIN_EIGENVALS, kind)
            check(ctx, g0, g1, pts, counts, win, L, seed, R.USE_INITIAL_FLOW, kind)
        check(ctx, g0, g1, pts, counts, win, L, None, R.GET_MIN_EIGENVALS, "eig")
    finally:
        ctx.close()


def test_criteria_clamps_and_thresholds(pkg, gpu_ctx):
    g0, g1, base = frames(pkg, 480, 640, 3)
    pts, truth = points(g0, base, 72, 15, 17)
    counts = np.array([72, 30, 72], np.int32)
    for lk in (dict(max_count=0, eps=0.03, min_eig_thr=1e-4), dict(max_count=300, eps=-1.0, min_eig_thr=1e-4), dict(max_count=3, eps=50.0, min_eig_thr=1e-4),
               dict(max_count=20, eps=0.03, min_eig_thr=5e-2)):
        for win, L in ((15, 2), (21, 1)):
            check(gpu_ctx, g0, g1, pts, counts, win, L, truth, R.USE_INITIAL_FLOW | R.GET_MIN_EIGENVALS, str(lk), lk)
            check(gpu_ctx, g0, g1, pts, counts, win, L, truth, R.USE_INITIAL_FLOW, str(lk), lk)


def _call_ex(ofk, ctx, g0, g1, pts, counts, win, L, init, flags):
    B, h, w = g0.shape
    S = pts.shape[1]
    nxt = np.zeros((B, S, 2), np.float32); st = np.zeros((B, S), np.uint8); err = np.zeros((B, S), np.float32)
    rc = ctx._L.ofk_lk_pyr_ex(ctx._h, ofk._p(g0), ofk._p(g1), B, h, w, ofk._p(pts), ofk._p(counts), S, win, L, 20, 0.03, 1e-4,
                              None if init is None else ofk._p(init), flags, ofk._p(nxt), ofk._p(st), ofk._p(err))
    return rc, nxt, st, err


def test_flags_zero_is_ofk_lk_pyr(pkg, ofk, gpu_ctx):
    g0, g1, base = frames(pkg, 480, 640, 3)
    for win in (15, 11, 21, 27):
        pts, truth = points(g0, base, 72, win, 23)
        counts = np.array([72, 9, 50], np.int32)
        want = gpu_ctx.lk_pyr(g0, g1, pts, counts, win=win, max_level=3)             # ofk_lk_pyr
        rc, nxt, st, err = _call_ex(ofk, gpu_ctx, g0, g1, pts, counts, win, 3, None, 0)
        assert rc == ofk.OK
        for b in range(3):
            n = counts[b]
            assert np.array_equal(bits(nxt[b, :n]), bits(want[0][b, :n])) and np.array_equal(st[b, :n], want[1][b, :n])
            assert np.array_equal(bits(err[b, :n]), bits(want[2][b, :n]))
        # init_pts without the flag are ignored, as OpenCV ignores nextPts
        rc, nxt2, st2, err2 = _call_ex(ofk, gpu_ctx, g0, g1, pts, counts, win, 3, truth, 0)
        assert rc == ofk.OK and np.array_equal(bits(nxt2), bits(nxt)) and np.array_equal(st2, st) and np.array_equal(bits(err2), bits(err))


def test_refusals(pkg, ofk, gpu_ctx):
    g0, g1, base = frames(pkg, 480, 640, 3)
    pts, truth = points(g0, base, 72, 15, 29)
    counts = np.array([72, 9, 50], np.int32)
    for bad in (np.nan, np.inf, -np.inf, 1.0000001e6, -2e6):
        seed = truth.copy(); seed[1, 8, 1] = bad               # inside counts[1] = 9
        rc, *_ = _call_ex(ofk, gpu_ctx, g0, g1, pts, counts, 15, 3, seed, ofk.LK_USE_INITIAL_FLOW)
        assert rc == ofk.E_INVALID, bad
        with pytest.raises(ofk.OfkError):
            gpu_ctx.lk_pyr(g0, g1, pts, counts, next_pts=seed, flags=ofk.LK_USE_INITIAL_FLOW)
    seed = truth.copy(); seed[1, 9, 0] = np.nan                 # beyond counts[1]: not a used coordinate
    assert _call_ex(ofk, gpu_ctx, g0, g1, pts, counts, 15, 3, seed, ofk.LK_USE_INITIAL_FLOW)[0] == ofk.OK
    assert _call_ex(ofk, gpu_ctx, g0, g1, pts, counts, 15, 3, None, ofk.LK_USE_INITIAL_FLOW)[0] == ofk.E_INVALID
    assert _call_ex(ofk, gpu_ctx, g0, g1, pts, counts, 15, 3, truth, 1)[0] == ofk.E_INVALID
    assert _call_ex(ofk, gpu_ctx, g0, g1, pts, counts, 15, 3, truth, 4 | 16)[0] == ofk.E_INVALID
    with pytest.raises(ValueError):
        gpu_ctx.lk_pyr(g0, g1, pts, counts, flags=ofk.LK_USE_INITIAL_FLOW)
    # the context still works after the refusals
    check(gpu_ctx, g0, g1, pts, counts, 15, 3, truth, R.USE_INITIAL_FLOW, "after refusals")


def test_predict_points_matches_the_numpy_predictor(pkg, ofk, gpu_ctx):
    rng = np.random.default_rng(31)
    B, S = 4, 300
    pts = np.stack([rng.uniform(-50, 2000, (B, S)), rng.uniform(-50, 1200, (B, S))], 2).astype(np.float32)
    counts = np.array([S, 0, 123, 299], np.int32)
    total = differ = 0
    for trial in range(6):
        sens = ofk.make_sensors(B, d=1.0, scaling=1 / 1920, cx=960.0, cy=540.0)
        sens[:, 0] = rng.uniform(0.3, 30, B); sens[:, 1:4] = rng.normal(0, 1, (B, 3)); sens[:, 4:7] = rng.normal(0, 0.1, (B, 3))
        sens[:, 22:25] = rng.normal(0, 0.1, (B, 3)); sens[:, 19] = 1 / rng.uniform(300, 4000, B); sens[:, 20:22] += rng.uniform(-30, 30, (B, 2))
        gain = (1.0, 0.5, 1 / 30, 2.0, 1.0, 1.0)[trial]
        if trial == 4:
            sens[0, 19] = 0.0; sens[2, 0] = 0.0; sens[3, 4] = np.nan       # fall back to the points
        if trial == 5:
            sens[0, 5] = 1e9; sens[2, 22] = np.inf; sens[3, 4:7] = 0; sens[3, 22:25] = 0
        for mode in (ofk.SEED_MODEL, ofk.SEED_ROTATION):
            got = gpu_ctx.predict_points(pts, counts, sens, mode, gain)
            for b in range(B):
                n = counts[b]
                want = R.predict(pts[b, :n], sens[b], mode, gain)
                gi = got[b, :n].view(np.int32).astype(np.int64); wi = want.view(np.int32).astype(np.int64)
                assert np.all(np.abs(gi - wi) <= 1), (trial, mode, b)      # at most one ulp (same sign: the bit patterns are ordered)
                total += gi.size; differ += int(np.sum(gi != wi))
                assert np.array_equal(bits(got[b, n:]), bits(pts[b, n:]))
                if trial == 4 or (trial == 5 and b in (0, 3)) or (trial == 5 and b == 2 and mode == ofk.SEED_MODEL):
                    assert np.array_equal(bits(got[b, :n]), bits(pts[b, :n])), (trial, mode, b)
    print(f"ofk_predict_points: {differ} of {total} values differ from the numpy predictor (each by one ulp)")
    with pytest.raises(ofk.OfkError):
        gpu_ctx.predict_points(pts, counts, sens, ofk.SEED_OFF, 1.0)
