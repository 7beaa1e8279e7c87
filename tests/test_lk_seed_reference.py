"""The test-side reference of the seeded LK (tests/lk_seed_reference.py) against the oracle, and the fast-manoeuvre experiment that
motivates seeding.  CPU only: it tests the reference the GPU tests compare against."""
import numpy as np
import pytest

from oracle import image_oracle as io, estimation_oracle as eo
import lk_seed_reference as R  # noqa: E402  (tests/lk_seed_reference.py)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def images(kind, h=120, w=160):
    rng = np.random.default_rng(5 if kind == "smooth" else 6)
    if kind == "smooth":
        yy, xx = np.mgrid[0:h, 0:w]
        a = 128 + 60 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 20 * np.sin((xx + yy) / 13.0)
        b = 128 + 60 * np.sin((xx - 1.3) / 9.0) * np.cos((yy - 0.8) / 7.0) + 20 * np.sin((xx + yy - 2.1) / 13.0)
        return np.clip(a, 0, 255).astype(np.uint8), np.clip(b, 0, 255).astype(np.uint8)
    a = rng.integers(0, 256, (h, w)).astype(np.uint8)
    a = io.pyr_down(np.kron(a, np.ones((2, 2), np.uint8)))            # correlated noise: trackable and full of contrast
    return a, np.roll(a, (1, 2), axis=(0, 1))


def border_points(h, w, rng, n=40):
    """Points near every border and corner, some outside, plus interior ones."""
    edge = [(-3.5, 10), (0.2, 0.3), (w - 1.2, 5.5), (w + 2.0, h / 2), (w / 2, -2.5), (w / 2, 0.4), (w / 2, h - 0.6), (w / 3, h + 3.0),
            (1.5, h - 1.5), (w - 1.5, h - 1.5), (w - 0.5, 0.5), (7.0, 7.0), (w - 8.0, h - 8.0)]
    inner = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], 1)
    return np.concatenate([np.array(edge), inner]).astype(np.float32)


@pytest.mark.parametrize("kind", ["smooth", "textured"])
@pytest.mark.parametrize("win", [3, 7, 15, 21, 31])
def test_plain_equals_the_oracle(kind, win):
    a, b = images(kind)
    pts = border_points(a.shape[0], a.shape[1], np.random.default_rng(win))
    for L in range(4):
        ref = io.lk_pyr(a, b, pts, win, L, 20, 0.03, 1e-4)
        assert same(R.lk_pyr(a, b, pts, win, L, 20, 0.03, 1e-4), ref), (kind, win, L)
        # a seed equal to the points is the plain call
        assert same(R.lk_pyr(a, b, pts, win, L, 20, 0.03, 1e-4, seed=pts, flags=R.USE_INITIAL_FLOW), ref), (kind, win, L)


@pytest.mark.parametrize("kind", ["smooth", "textured"])
def test_min_eigenvalue_flag_contract(kind):
    a, b = images(kind)
    rng = np.random.default_rng(9)
    pts = border_points(a.shape[0], a.shape[1], rng)
    seed = pts + rng.uniform(-6, 6, pts.shape).astype(np.float32)
    for win in (7, 15, 21):
        for L in (0, 2):
            for fl, sd in ((0, None), (R.USE_INITIAL_FLOW, seed)):
                n0, s0, e0 = R.lk_pyr(a, b, pts, win, L, 20, 0.03, 1e-3, seed=sd, flags=fl)
                n1, s1, e1 = R.lk_pyr(a, b, pts, win, L, 20, 0.03, 1e-3, seed=sd, flags=fl | R.GET_MIN_EIGENVALS)
                assert same((n0, s0), (n1, s1))
                # level-0 minEig, from the oracle's own derivative image: exact integer sums, the f32 formula of orc_lk_pyr
                der = io.scharr(a).astype(np.int64)
                half = np.float32((win - 1) * 0.5)
                got_lost_with_value = 0
                for p in range(len(pts)):
                    px = np.float32(pts[p, 0]) - half; py = np.float32(pts[p, 1]) - half
                    ix, iy = int(np.floor(px)), int(np.floor(py))
                    if ix < -win or ix >= a.shape[1] or iy < -win or iy >= a.shape[0]:
                        assert e1[p, 0] == 0 and s1[p, 0] == 0
                        continue
                    fa, fb = np.float32(px - np.float32(ix)), np.float32(py - np.float32(iy))
                    one = np.float32(1)
                    w = [int(np.rint((one - fa) * (one - fb) * np.float32(16384))), int(np.rint(fa * (one - fb) * np.float32(16384))),
                         int(np.rint((one - fa) * fb * np.float32(16384)))]
                    w.append(16384 - sum(w))
                    pad = np.zeros((a.shape[0] + 2 * win + 4, a.shape[1] + 2 * win + 4, 2), np.int64)
                    pad[win + 2:win + 2 + a.shape[0], win + 2:win + 2 + a.shape[1]] = der
                    y0, x0 = iy + win + 2, ix + win + 2
                    blk = lambda dy, dx: pad[y0 + dy:y0 + dy + win, x0 + dx:x0 + dx + win]
                    g = (blk(0, 0) * w[0] + blk(0, 1) * w[1] + blk(1, 0) * w[2] + blk(1, 1) * w[3] + (1 << 13)) >> 14
                    A11 = np.float32(float((g[..., 0] ** 2).sum()) * 2.0 ** -20); A22 = np.float32(float((g[..., 1] ** 2).sum()) * 2.0 ** -20)
                    A12 = np.float32(float((g[..., 0] * g[..., 1]).sum()) * 2.0 ** -20)
                    dd = A11 - A22
                    me = (A22 + A11 - np.sqrt(dd * dd + np.float32(4) * A12 * A12)) / np.float32(2 * win * win)
                    assert bits(np.float32(me)) == bits(e1[p, 0]), (win, L, p)
                    got_lost_with_value += int(s1[p, 0] == 0 and e1[p, 0] != 0)
                if kind == "smooth" and win == 7:
                    assert got_lost_with_value > 0        # the value is reported whatever the status becomes


@pytest.mark.parametrize("row", R.ROWS, ids=[r[0] for r in R.ROWS])
def test_experiment_rows_reproduce(row):
    name, v, omega, expect, inside, (fmed, fmax) = row
    e = R.experiment_pair(name)
    sens = R.experiment_sensors(e["pair"])
    mag = np.linalg.norm(e["flow"], axis=1)
    assert len(e["pts"]) == 300 and round(float(np.median(mag)), 1) == fmed and round(float(mag.max()), 1) == fmax
    plain3 = R.lk_pyr(e["g0"], e["g1"], e["pts"], max_level=3, **R.EXP_LK)
    plain0 = R.lk_pyr(e["g0"], e["g1"], e["pts"], max_level=0, **R.EXP_LK)
    seed = R.predict(e["pts"], sens)
    seeded0 = R.lk_pyr(e["g0"], e["g1"], e["pts"], max_level=0, seed=seed, flags=R.USE_INITIAL_FLOW, **R.EXP_LK)
    got = tuple(R.good_points(e, r[0], r[1]) for r in (plain3, plain0, seeded0))
    print(name, got)
    assert got == tuple((g, inside) for g in expect)
    assert got[2][0] >= R.SEEDED_MIN_GOOD * inside
    if name in R.LARGE_MOTION:
        assert got[1][0] <= R.PLAIN_MAX_GOOD * inside
    # the oracle agrees on the plain columns (the restatement adds nothing there)
    assert same(plain3, io.lk_pyr(e["g0"], e["g1"], e["pts"], 15, 3, 20, 0.03, 1e-4))
    # seeding with the points themselves is the plain call, bit for bit
    assert same(R.lk_pyr(e["g0"], e["g1"], e["pts"], max_level=3, seed=e["pts"], flags=R.USE_INITIAL_FLOW, **R.EXP_LK), plain3)
    # rotation-only seeds: the same conditions where the motion is rotational; no help against a translation
    rot = R.predict(e["pts"], sens, mode=R.SEED_ROTATION)
    r0 = R.lk_pyr(e["g0"], e["g1"], e["pts"], max_level=0, seed=rot, flags=R.USE_INITIAL_FLOW, **R.EXP_LK)
    gr = R.good_points(e, r0[0], r0[1])[0]
    if name in R.ROTATION_ROWS:
        assert gr >= R.SEEDED_MIN_GOOD * inside
    if name == "translation":
        assert gr == 0


@pytest.mark.parametrize("row", R.ROWS, ids=[r[0] for r in R.ROWS])
def test_predictor_is_the_flow_model(row):
    name = row[0]
    e = R.experiment_pair(name)
    pair = e["pair"]
    p64 = e["pts"].astype(np.float64)
    x = (p64 - [pair["cx"], pair["cy"]]) * pair["scaling"]
    want = p64 + eo.generate_test_data(x, pair["v"], pair["omega"], pair["d"], pair["n"]) / pair["scaling"]
    got = R.predict_f64(e["pts"], pair["d"], pair["n"], pair["omega"], pair["v"], pair["scaling"], pair["cx"], pair["cy"])
    assert np.max(np.abs(got - want) / np.abs(want)) <= 1e-12
    seeds = R.predict(e["pts"], R.experiment_sensors(pair))
    assert np.array_equal(seeds, got.astype(np.float32))
    dist = np.linalg.norm(seeds.astype(np.float64) - (p64 + e["flow"]), axis=1).max()
    print(name, "predictor vs true flow, max px:", dist)
    assert dist < (3.0 if name == "pitchroll" else 0.25)
    if name in R.ROTATION_ROWS:                     # omega alone leaves out a translational flow of <= 3 px in these rows
        rot = R.predict(e["pts"], R.experiment_sensors(pair), mode=R.SEED_ROTATION)
        want_rot = p64 + eo.generate_test_data(x, np.zeros(3), pair["omega"], pair["d"], pair["n"]) / pair["scaling"]
        assert np.max(np.abs(rot.astype(np.float64) - want_rot)) <= 1e-4


def test_predictor_falls_back_to_the_point():
    pts = np.array([[10.5, 20.25], [300.0, 200.0]], np.float32)
    s = R.experiment_sensors(dict(d=1.0, n=(0, 0, 1), omega=(0.01, 0.02, 0.03), scaling=1 / 640, cx=320.0, cy=240.0, v=(0.01, 0, 0)))
    for k, val in ((19, 0.0), (0, 0.0), (4, np.nan), (5, np.inf), (6, 1e9)):
        t = s.copy(); t[k] = val
        assert np.array_equal(R.predict(pts, t), pts), k
    assert not np.array_equal(R.predict(pts, s), pts)
    assert np.array_equal(R.predict(pts, s, gain=0.0), pts)


def test_stream_loop_helper_equals_the_stream_oracle_with_seeding_off(pkg):
    """The stream loop with its tracker plug (tests/stream_oracle.py::NodeLoop) gives what oracle_stream gave while it was a loop of
    its own (tests/golden/stream_loops.npz, recorded from it), and the restated tracker in the plug changes nothing."""
    import os
    from of_amd import synth
    from of_amd.pipeline import PipelineConfig
    from stream_oracle import NodeLoop, oracle_stream
    cfg = PipelineConfig(max_corners=60, quality=0.04, min_distance=9, block_size=7, win=15, max_level=2, max_count=20, eps=0.03)
    frames, info = synth.render_sequence(240, 320, 77, 5, v=(0.03, 0.012, 0.0), omega=(0.0, 0.0, 0.01), d=1.0)
    s = R.experiment_sensors(info, v_prior=(0, 0, 0))
    pinned = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_loops.npz"))
    redetected = False
    for min_feat in (59, 10):
        first, steps = oracle_stream(frames, cfg, s, min_feat, 12)
        rec = {f: pinned[f"plain-{min_feat}/{f}"] for f in ("first", "v", "v.size", "tracks", "tracks.size", "n_old", "n_tracked")}
        first2 = rec["first"]
        steps2 = list(zip([None if n < 0 else v for n, v in zip(rec["v.size"], np.split(rec["v"], np.cumsum(np.maximum(rec["v.size"], 0))[:-1]))],
                          [t.reshape(-1, 2) for t in np.split(rec["tracks"], np.cumsum(rec["tracks.size"])[:-1])], rec["n_old"], rec["n_tracked"]))
        assert np.array_equal(first, first2) and len(steps) == len(steps2)
        for a, b in zip(steps, steps2):
            assert (a[0] is None) == (b[0] is None) and (a[0] is None or np.array_equal(a[0], b[0]))
            assert np.array_equal(bits(a[1].astype(np.float32)), bits(b[1].astype(np.float32))) and a[2:] == tuple(b[2:])
            redetected = redetected or len(a[1]) > a[3]
        # the restated tracker without a seed is the oracle's tracker, so the loop does not change either
        ref_lk = lambda g0, g1, old: R.lk_pyr(g0, g1, old, cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr)
        loop = NodeLoop(frames[0], cfg, min_feat, 12, lk=ref_lk)
        steps3 = [loop.step(frames[t], s)["tracks"] for t in range(1, len(frames))]
        assert all(np.array_equal(a[1], b) for a, b in zip(steps, steps3))
    assert redetected
