"""CPU-only: the numpy restatement of the exclusion zones (tests/zones_reference.py) against the package's own host helpers
(of_library._hull, _fill_convex, distancecluster), known answers of the rules, and what the zones achieve on the restated stream loop."""
import math

import numpy as np

import zones_reference as zr


def test_hull_equals_of_library(pkg):
    from of_amd import of_library as ol
    rng = np.random.default_rng(5)
    cases = [rng.integers(0, 40, (n, 2)) for n in (1, 2, 3, 4, 7, 30, 200)]
    cases += [np.array([[3, 3]] * 3), np.array([[0, 0], [5, 5], [10, 10]]), np.array([[0, 0], [4, 0], [4, 0], [0, 0]]),
              np.array([[2, 9], [2, 1], [2, 5]]), np.array([[0, 0], [10, 0], [10, 10], [0, 10], [5, 5], [5, 0]])]
    for pts in cases:
        ours, theirs = zr.hull(pts), ol._hull(pts)
        assert np.array_equal(np.array(ours, np.float64).reshape(-1, 2), np.asarray(theirs, np.float64).reshape(-1, 2)), pts
    ring = [(int(round(300 + 200 * math.cos(2 * math.pi * k / 40))), int(round(230 + 200 * math.sin(2 * math.pi * k / 40)))) for k in range(40)]
    assert len(zr.hull(ring)) > zr.ZONE_VERTS
    assert len(zr.hull(ring)) == 40 and zr.zone_vertices(ring) == [(100, 30), (500, 30), (500, 430), (100, 430)]


def test_shape_at_radius_0_equals_fill_convex(pkg):
    from of_amd import of_library as ol
    rng = np.random.default_rng(6)
    yy, xx = np.mgrid[0:48, 0:64]
    for n in (1, 2, 3, 5, 12, 40):
        for _ in range(4):
            V = zr.hull(np.stack([rng.integers(-5, 70, n), rng.integers(-5, 53, n)], 1))
            theirs = np.ones((48, 64), np.uint8)
            ol._fill_convex(theirs, np.array(V, dtype="int32"), 0)
            ours = np.where(zr.inside(xx, yy, V, 0), 0, 1).astype(np.uint8)
            assert np.array_equal(ours, theirs), V
    for V in ([(10, 10), (30, 10)], [(5, 5), (25, 45)], [(7, 9)]):       # a segment's lattice points; a point
        theirs = np.ones((48, 64), np.uint8)
        ol._fill_convex(theirs, np.array(V, dtype="int32"), 0)
        assert np.array_equal(np.where(zr.inside(xx, yy, V, 0), 0, 1).astype(np.uint8), theirs), V
    disc = np.ones((48, 64), np.uint8)
    ol._disc(disc, 20, 22, 9, 0)
    assert np.array_equal(np.where(zr.inside(xx, yy, [(20, 22)], 9), 0, 1).astype(np.uint8), disc)


def test_labels_are_distanceclusters_components_in_logarithmic_sweeps(pkg):
    from of_amd import of_library as ol
    rng = np.random.default_rng(7)
    for n, link in ((1, 5), (12, 6), (60, 9), (150, 7)):
        pos = rng.integers(0, 120, (n, 2)).astype(np.int64)
        lab, sweeps = zr.labels(pos, link)
        clusters, _ = ol.distancecluster(np.zeros((0, 2)), pos, link, [])
        assert sorted(sorted(c) for c in clusters) == sorted(sorted(np.nonzero(lab == r)[0].tolist()) for r in set(lab.tolist()))
        assert all(lab[r] == r for r in set(lab.tolist())) and all(lab[i] <= i for i in range(n))
    # a chain of 2000 points: a pass of the hooking leaves at most every other tree unhooked, whatever the index order
    path = np.stack([3 * np.arange(2000), np.zeros(2000, np.int64)], 1)
    for order in (np.arange(2000)[::-1], rng.permutation(2000), np.arange(2000)):
        lab, sweeps = zr.labels(path[order], 4)
        assert not lab.any() and sweeps <= math.ceil(math.log2(2000)) + 1, sweeps


def test_rules_on_known_answers():
    s = dict(zr.DEFAULT, link=10, min_members=3, radius=2, ttl=3, max_zones=2)
    t = zr.Table()
    old = np.array([[10.9, 10.2], [14, 10], [12, 16.7], [40, 40], [12, 12], [60, 5]], np.float32)
    new = old + np.array([[1, 0], [2, 0], [3, 0], [9, 9], [5, 5], [0, 0]], np.float32)
    status = np.array([1, 1, 1, 1, 0, 1], np.uint8); keep = np.array([0, 0, 0, 0, 0, 1], np.uint8)
    mask = zr.step(t, s, old, new, status, keep, 48, 64)
    # the lost point (status 0) and the kept one take no part; (40, 40) is alone: below min_members
    assert t.zones[0, :3].tolist() == [2, 3, 3] and t.zones[0, 3:9].tolist() == [10, 10, 14, 10, 12, 16] and not t.zones[1].any()
    assert t.motion[0].tolist() == [2.0, 0.0, 2.0, 0.0] and t.stats.tolist() == [1, 1, 0, 0, 4, 0, 2, 0]
    assert mask[12, 12] == 0 and mask[8, 10] == 0 and mask[7, 10] == 1 and mask[40, 40] == 1 and mask[10, 17] == 1
    # next step: a reject inside the moved zone refreshes it and does not cluster; the zone was at x + 2
    mask = zr.step(t, s, np.array([[14, 12], [30, 30]], np.float32), np.zeros((2, 2), np.float32), [1, 1], [0, 0], 48, 64)
    assert t.zones[0, 0] == 2 and t.stats.tolist() == [1, 0, 1, 0, 2, 1, 1, 0] and t.motion[0, :2].tolist() == [4.0, 0.0]
    assert mask[10, 18] == 0 and mask[10, 9] == 1
    for _ in range(2):
        zr.step(t, s, np.zeros((0, 2)), np.zeros((0, 2)), [], [], 48, 64)
    assert not t.zones.any() and not t.motion.any() and t.stats[0] == 0


def run_loops(pkg, seed, nf=12):
    from of_amd import synth, ofk
    from of_amd.pipeline import PipelineConfig
    import robust_reference as rr
    import robust_stream_oracle as rso
    from stream_oracle import NodeLoop
    h, w = 480, 640
    cfg = PipelineConfig(max_corners=200, quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)
    frames, info = rso.sequence(synth, h, w, seed, nf)
    sr = ofk.make_sensors(1, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"])[0]
    runs = {}
    for zones in (False, True):
        kw = dict(solve=rso.robust_solver(0, True, False))
        loop = zr.ZoneNodeLoop(frames[0], cfg, 199, 15, **kw) if zones else NodeLoop(frames[0], cfg, 199, 15, **kw)
        rows = []
        for t in range(1, nf):
            o = loop.step(frames[t], sr)
            redetected = o["redetected"] if zones else o["n_old"] <= 199 and o["n_old"] < cfg.max_corners
            rows.append(dict(t=t, share=float(np.mean(rso.on_object(o["tracks"], t))), dropped=o["n_tracked"] - int(np.count_nonzero(o["keep"])),
                             tracks=len(o["tracks"]), err=rr.rel_err(o["v"], info["v"]), redetected=bool(redetected)))
        runs[zones] = rows
    return runs


def test_zones_keep_the_redetection_off_the_moving_object(pkg):
    """The experiment of the reference's docstring: seeds 900 and 901, 12 frames, min_features 199, the default setting."""
    import robust_reference as rr
    for seed in (900, 901):
        runs = run_loops(pkg, seed)
        plain, zoned = runs[False], runs[True]
        for name, rows in (("without", plain), ("with", zoned)):
            late = [r["share"] for r in rows if r["redetected"] and r["t"] >= 3]
            print(f"seed {seed} {name} zones: dropped {sum(r['dropped'] for r in rows)}, re-detections {sum(r['redetected'] for r in rows)}, "
                  f"share behind a re-detection {min(r['share'] for r in rows if r['redetected']):.3f}-{max(r['share'] for r in rows if r['redetected']):.3f}, "
                  f"from step 3 on {min(late):.3f}-{max(late):.3f}, tracks {min(r['tracks'] for r in rows)}-{max(r['tracks'] for r in rows)}, "
                  f"velocity error {min(r['err'] for r in rows):.4f}-{max(r['err'] for r in rows):.4f}")
        assert any(z["redetected"] and z["t"] >= 3 for z in zoned)
        for p, z in zip(plain, zoned):
            assert z["err"] <= rr.ROBUST_MAX and p["err"] <= rr.ROBUST_MAX, (seed, z["t"])
            if z["redetected"] and z["t"] >= 3:
                assert z["share"] < p["share"], (seed, z["t"], z["share"], p["share"])
        assert sum(z["dropped"] for z in zoned) < sum(p["dropped"] for p in plain), seed
