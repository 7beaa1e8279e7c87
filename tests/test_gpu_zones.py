"""GPU: the exclusion zones (ofk_set_zones) against the numpy restatement of tests/zones_reference.py, bit for bit.

(1) ofk_zones_step, the stage entry, on constructed rejects: mask, table and statistics after every step.
(2) FlowStream.step / step_fused (append- and replace-mode re-detection) on the moving-object sequence against ZoneNodeLoop, as
    tests/test_gpu_robust_pipeline.py compares its drop streams: tracks, counts and the zone table equal.
(3) never set == set and switched off again."""
import math

import numpy as np
import pytest

import robust_reference as rr
import robust_stream_oracle as rso
import zones_reference as zr
from point_stage_helpers import bits
from zones_edge_cases import NONE, rejects, run_steps

pytestmark = pytest.mark.gpu

H, W, B, S = 480, 640, 3, 512


@pytest.fixture(scope="module")
def zctx(ofk):
    c = ofk.Context(0, W, H, B, S, 2)
    yield c
    c.close()


def test_few_rejects_collinear_and_identical_ones(zctx):
    s = dict(link=10, min_members=3, radius=4, ttl=5)
    tables, mask = run_steps(zctx, s, [[NONE, rejects([[20.5, 20.5]]), rejects([[20, 20], [24, 23]])]], 48, 64)
    assert not any(t.zones.any() for t in tables) and [int(t.stats[4]) for t in tables] == [0, 1, 2] and mask.all()
    tables, mask = run_steps(zctx, s, [[rejects([[10, 10], [16, 13], [22, 16]], (1.5, -0.25)), rejects([[30.2, 30.9]] * 3, (0.0, 2.0)),
                                        rejects([[5, 5], [9, 5], [9, 5], [13, 5], [5, 5]])]], 48, 64)
    assert [int(t.zones[0, 1]) for t in tables] == [2, 1, 2] and [int(t.zones[0, 2]) for t in tables] == [3, 3, 5]      # capsule, disc, capsule
    assert tables[0].zones[0, 3:7].tolist() == [10, 10, 22, 16] and tables[1].zones[0, 3:5].tolist() == [30, 30]
    assert mask[0, 13, 16] == 0 and mask[1, 30, 34] == 0 and mask[1, 30, 35] == 1 and mask[2, 5, 17] == 0 and mask[2, 5, 18] == 1


@pytest.mark.parametrize("gap", [0, 1], ids=["at-link", "below-link"])
def test_two_groups_at_and_just_below_the_link_distance(zctx, gap):
    link = 12
    a = np.array([[100, 100], [104, 108], [108, 101]], np.float32)
    for axis in (0, 1):
        shift = np.zeros(2, np.float32); shift[axis] = 8 + link - gap        # nearest members: link - gap apart on that axis, a few pixels on the other
        tables, _ = run_steps(zctx, dict(link=link, min_members=3, radius=3, ttl=4), [[rejects(np.concatenate([a, a + shift]))]], H, W)
        assert int(tables[0].stats[1]) == (2 if gap == 0 else 1), (axis, tables[0].stats)


def snake(n):
    pts, x, y, d = [], 10, 10, 1
    while len(pts) < n:
        pts.append((x, y))
        if (d == 1 and x + 3 > 600) or (d == -1 and x - 3 < 10):
            pts += [(x + 3 * d, y + 3), (x + 3 * d, y + 6)]; y += 9; d = -d
        else:
            x += 3 * d
    return np.array(pts[:n], np.float32)


def test_snake_against_its_index_order(zctx):
    p = snake(300)
    rng = np.random.default_rng(3)
    lab, _ = zr.labels(p.astype(np.int64), 4)
    d = np.abs(p[:, None] - p[None]).max(-1)
    assert not lab.any() and ((d < 4).sum(1) <= 3).all()        # one component, and a path: nobody has more than two neighbours
    tables, _ = run_steps(zctx, dict(link=4, min_members=3, radius=2, ttl=3), [[rejects(p[::-1] + 0.5, (0.25, 0.5)), rejects(p[rng.permutation(300)]), rejects(p)]], H, W)
    for t in tables:
        assert t.stats[1] == 1 and t.zones[0, 2] == 300 and 1 <= t.stats[6] <= math.ceil(math.log2(300)) + 1, t.stats
    print("label sweeps of the 300-point chain (reversed, shuffled, in order):", [int(t.stats[6]) for t in tables])


def test_257_rejects_in_one_stream_of_three(zctx):
    rng = np.random.default_rng(11)
    p = np.stack([rng.uniform(0, W, 257), rng.uniform(0, H, 257)], 1).astype(np.float32)
    mask_in = (rng.random((1, B, H, W)) < 0.9).astype(np.uint8)
    old, new, st, kp = rejects(p, (0.0, 0.0))
    new = old + rng.normal(0, 2, old.shape).astype(np.float32)
    st[::17] = 0                                                 # lost points
    kp[5::29] = 1                                                # kept ones
    tables, mask = run_steps(zctx, dict(link=30, min_members=3, radius=6, ttl=9), [[NONE, (old, new, st, kp), NONE]], H, W, masks=mask_in)
    assert tables[1].stats[4] == int(np.count_nonzero((st == 1) & (kp == 0))) and tables[1].stats[1] >= 1 and not tables[0].zones.any()
    assert np.array_equal(mask[0], mask_in[0, 0]) and not mask[1][mask_in[0, 1] == 0].any()


def test_circle_of_40_becomes_its_bounding_box(zctx):
    ring = [(round(300 + 200 * math.cos(2 * math.pi * k / 40)) + 0.75, round(230 + 200 * math.sin(2 * math.pi * k / 40)) + 0.25) for k in range(40)]
    tables, mask = run_steps(zctx, dict(link=48, min_members=3, radius=5, ttl=2), [[rejects(ring, (-3.5, 2.5))], [NONE], [NONE]], H, W)
    assert not tables[0].zones.any()                             # expired behind the second step


def test_17_clusters_with_16_slots(zctx):
    p = np.concatenate([[[20 + 35 * k, 30 + 20 * (k % 3)], [24 + 35 * k, 37 + 20 * (k % 3)], [28 + 35 * k, 31 + 20 * (k % 3)]] for k in range(17)]).astype(np.float32)
    tables, _ = run_steps(zctx, dict(link=10, min_members=3, radius=2, ttl=4, max_zones=16), [[rejects(p, (1.0, 0.0)), rejects(p[:21])], [rejects(p + [0, 200])]], H, W)
    assert tables[0].stats.tolist()[:4] == [16, 17, 0, 17]      # second step: every insert replaces a zone of the first
    tables, _ = run_steps(zctx, dict(link=10, min_members=3, radius=2, ttl=4, max_zones=5), [[rejects(p)]], H, W)
    assert tables[0].stats.tolist()[:4] == [5, 17, 0, 12] and [int(z[3]) for z in tables[0].zones[:5]] == [20 + 35 * k for k in (16, 1, 2, 3, 4)]      # equal ttl: every insert past the fifth takes slot 0


def test_zone_leaves_the_image_and_expires(zctx):
    steps = [[rejects([[50, 20], [56, 30], [60, 22]], (4.0, -1.5)), rejects([[3, 40], [9, 44], [5, 46]], (-0.5, 0.75))]] + [[NONE, NONE]] * 7
    tables, mask = run_steps(zctx, dict(link=12, min_members=3, radius=3, ttl=7), steps, 48, 64)
    assert not tables[0].zones.any() and not tables[1].zones.any() and mask.all()


@pytest.mark.parametrize("radius", [0, 255])
def test_radius_0_and_255(zctx, radius):
    steps = [[rejects([[300, 200], [340, 260], [280, 250], [310, 230]], (2.5, 1.5)), rejects([[10, 10], [14, 14], [18, 18]]), rejects([[630, 470]] * 3)], [NONE] * 3]
    run_steps(zctx, dict(link=70, min_members=3, radius=radius, ttl=3), steps, H, W)


def test_refresh_by_a_reject_inside_two_overlapping_zones(zctx):
    a = np.array([[100, 100], [110, 104], [104, 110]], np.float32)
    steps = [[rejects(np.concatenate([a, a + [30, 0]]))], [NONE], [rejects([[122, 104], [400, 300]])], [NONE]]
    tables, _ = run_steps(zctx, dict(link=20, min_members=3, radius=12, ttl=4), steps, H, W)
    # step 2's first reject lies in both zones (both refreshed, ttl back to 4), the second is alone: ttl 4 - 1 - 1 behind step 3
    assert tables[0].zones[:3, 0].tolist() == [2, 2, 0]


def test_lost_points_are_ignored(zctx):
    old = np.array([[100, 100], [104, 108], [108, 101], [200, 200], [204, 208], [208, 201]], np.float32)
    st = np.array([0, 0, 0, 1, 1, 1], np.uint8); kp = np.zeros(6, np.uint8)
    tables, _ = run_steps(zctx, dict(link=12, min_members=3, radius=3, ttl=4), [[(old, old + 1, st, kp), (old, old + 1, np.array([2, 1, 1, 1, 1, 0], np.uint8), np.array([0, 0, 0, 1, 0, 0], np.uint8))]], H, W)
    assert tables[0].stats.tolist()[:5] == [1, 1, 0, 0, 3] and tables[0].zones[0, 3] == 200 and tables[1].stats.tolist()[:5] == [0, 0, 0, 0, 3]


CFG = dict(max_corners=200, quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03,
           robust="tukey", robust_c=rso.SETTING["c"], robust_iters=rso.SETTING["iters"], robust_hypotheses=rso.SETTING["hypotheses"],
           robust_seed=rso.SETTING["seed"], robust_drop=True)
_seq = {}


def sequences(nf):
    from of_amd import synth
    if nf not in _seq:
        _seq[nf] = [rso.sequence(synth, H, W, 900 + b, nf) for b in range(2)]
    return _seq[nf]


@pytest.mark.parametrize("kind", ["step", "fused", "replace"])
def test_stream_steps_with_zones(pkg, ofk, kind):
    from of_amd.pipeline import FlowStream, PipelineConfig, FusionConfig
    nf, nb, min_feat, radius = 8, 2, 199, 15
    cfg = PipelineConfig(zones="hull", **CFG)
    seqs = sequences(nf)
    frames = np.stack([s[0] for s in seqs]); info = seqs[0][1]
    sensors = ofk.make_sensors(nb, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"])
    fusion = None if kind == "step" else FusionConfig(use_imu=False, redetect_replace=kind == "replace")
    fs = FlowStream(W, H, batch=nb, cfg=cfg, min_features=min_feat, mask_radius=radius, fusion=fusion)
    try:
        tracks, counts = fs.begin(frames[:, 0])
        loops = [zr.ZoneNodeLoop(frames[b, 0], cfg, min_feat, radius, replace=kind == "replace", solve=rso.robust_solver(b, True, kind != "step")) for b in range(nb)]
        for b in range(nb):
            assert counts[b] == len(loops[b].tracks) and np.array_equal(tracks[b, :counts[b]], loops[b].tracks)
        inserted = refreshed = masked = 0
        for t in range(1, nf):
            if kind == "step":
                rec, tracks, counts = fs.step(frames[:, t], sensors)
            else:
                rec, fused, tracks, counts = fs.step_fused(frames[:, t], sensors)
            got = fs.zones()
            for b in range(nb):
                o = loops[b].step(frames[b, t], sensors[b])
                tag = (kind, t, b)
                assert o["gap"] >= 1e-6 and o["near"] == 0, tag
                assert rec[b, 12] == o["n_old"] and rec[b, 13] == o["n_tracked"] and rec[b, 11] == o["used"] and counts[b] == len(o["tracks"]), \
                    (tag, rec[b, 11:14], o["n_old"], o["n_tracked"], o["used"], counts[b], len(o["tracks"]))
                assert np.array_equal(bits(tracks[b, :counts[b]]), bits(o["tracks"].astype(np.float32))), tag
                np.testing.assert_allclose(rec[b, :3], o["v"], rtol=1e-8, atol=1e-12, err_msg=str(tag))
                z = o["zones"]
                assert np.array_equal(got["stats"][b], z.stats), (tag, got["stats"][b], z.stats)
                assert np.array_equal(got["zones"][b], z.zones) and np.array_equal(bits(got["motion"][b]), bits(z.motion)), tag
                if kind != "replace":
                    assert rr.rel_err(rec[b, :3], info["v"]) <= rr.ROBUST_MAX, tag
                inserted += int(z.stats[1]); refreshed += int(z.stats[2]); masked += int(o["redetected"] and z.stats[0] > 0)
        print(f"{kind}: zones inserted {inserted}, refreshed {refreshed}, re-detections behind a zone mask {masked}")
        assert inserted > 0 and masked > 0 and (refreshed > 0 or kind == "replace")     # the replaced tracks are seldom rejected where a zone stands
    finally:
        fs.close()


def test_never_set_equals_set_and_switched_off(pkg, ofk):
    from of_amd.pipeline import FlowStream, PipelineConfig, FusionConfig
    nf = 5
    cfg = PipelineConfig(**CFG)
    seqs = sequences(8)
    frames = np.stack([s[0] for s in seqs])[:, :nf]; info = seqs[0][1]
    sensors = ofk.make_sensors(2, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"])
    for fused in (False, True):
        res = []
        for touch in ("never", "off-again", "on"):
            fs = FlowStream(W, H, batch=2, cfg=cfg, min_features=199, mask_radius=15, fusion=FusionConfig(use_imu=False) if fused else None)
            try:
                if touch == "on":
                    fs.ctx.set_zones(mode="hull")
                fs.begin(frames[:, 0])
                steps = []
                for t in range(1, nf):
                    if touch == "off-again" and t == 2:          # on and off again between two steps: nothing of it survives
                        fs.ctx.set_zones(mode="hull")
                        fs.ctx.set_zones(None)
                        assert fs.ctx.get_zones().mode == ofk.ZONES_OFF
                    out = fs.step_fused(frames[:, t], sensors) if fused else fs.step(frames[:, t], sensors)
                    steps.append((out[0], out[-2], out[-1]))
                res.append(steps)
            finally:
                fs.close()
        for (r0, t0, c0), (r1, t1, c1) in zip(res[0], res[1]):
            assert np.array_equal(c0, c1) and np.array_equal(bits(t0), bits(t1)) and np.array_equal(bits(r0), bits(r1)), fused
        assert any(not np.array_equal(bits(a[1]), bits(b[1])) for a, b in zip(res[0], res[2])), fused       # and on, they change the tracks
