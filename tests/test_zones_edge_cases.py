"""CPU-only: what stands behind tests/test_gpu_zones_edges.py.  (1) zones_reference.inside, with its |cross| <= 2^25 guard, against
rule 5 in unbounded Python integers without one; (2) known answers of rule 5's rounding and rule 1's clamp at their limits; (3) for
every case of tests/zones_edge_cases.py the condition that makes it a test of its edge, on the reference alone."""
import numpy as np
import pytest

import zones_edge_cases as ze
import zones_reference as zr


def inside_exact(px, py, V, r):
    """Rule 5 as include/ofk.h states it, in Python integers: no bound on any product, no guard."""
    n = len(V)
    if n == 0:
        return False
    conv, hit = n >= 3, False
    for i in range(1 if n <= 2 else n):
        (ax, ay), (bx, by) = V[i], V[(i + 1) % n]
        ex, ey, qx, qy = bx - ax, by - ay, px - ax, py - ay
        cr, t, L = ex * qy - ey * qx, qx * ex + qy * ey, ex * ex + ey * ey
        conv = conv and cr >= 0
        hit = hit or qx * qx + qy * qy <= r * r or (px - bx) ** 2 + (py - by) ** 2 <= r * r or (0 < t < L and cr * cr <= r * r * L)
    return hit or conv


def test_inside_with_its_guard_equals_exact_arithmetic():
    rng = np.random.default_rng(25)
    cases = guarded = hits = 0
    for k in range(2000):
        n = (1, 2, 3, 4, 7)[k % 5]
        hull = zr.hull(rng.integers(-32768, 32768, (n, 2)))
        off = ((0, 0), (1 << 20, -(1 << 20)), tuple(int(v) for v in rng.integers(-(1 << 20), (1 << 20) + 1, 2)))[k % 3]
        V = [(x + off[0], y + off[1]) for x, y in hull]
        r = (0, 1, 20, 255)[(k // 5) % 4]
        px, py = [int(v) for v in rng.integers(-32768, 32768, 5)], [int(v) for v in rng.integers(-32768, 32768, 5)]
        for _ in range(5):                                       # within radius + 1 of a point of a random edge
            i = int(rng.integers(len(V)))
            (ax, ay), (bx, by) = V[i], V[(i + 1) % len(V)]
            u = rng.random()
            px.append(round(ax + u * (bx - ax)) + int(rng.integers(-r - 1, r + 2))); py.append(round(ay + u * (by - ay)) + int(rng.integers(-r - 1, r + 2)))
        got = zr.inside(px, py, V, r)
        for x, y, g in zip(px, py, got):
            want = inside_exact(x, y, V, r)
            assert bool(g) == want, (V, r, x, y)
            hits += want
            guarded += any(abs((V[(i + 1) % len(V)][0] - V[i][0]) * (y - V[i][1]) - (V[(i + 1) % len(V)][1] - V[i][1]) * (x - V[i][0])) > 1 << 25 for i in range(len(V)))
        cases += len(px)
    print(f"{cases} pixels, {hits} inside, {guarded} with a |cross| above 2^25")
    assert cases == 20000 and guarded > 2000 and 2000 < hits < 18000


def test_shifted_rounds_half_to_even_and_saturates():
    t = zr.Table()
    t.zones[0, :5] = 3, 1, 3, 10, -10
    nan, inf = np.float32("nan"), np.float32("inf")
    for off, want in ((0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0), (-1.5, -2), (-2.5, -2), (3e6, 1 << 20), (-3e6, -(1 << 20)), (nan, -(1 << 20)), (inf, 1 << 20),
                      (-inf, -(1 << 20)), (1048576.5, 1 << 20), (-27001.5, -27002), (7000.5, 7000)):
        t.motion[0, :2] = off, -off
        v = zr.shifted(t, 0)
        assert v.dtype == np.int64 and v[0, 0] == 10 + want, (off, v)
        assert v[0, 1] == -10 + (-(1 << 20) if np.isnan(off) else -want), (off, v)


def test_positions_clamp_then_truncate():
    nan, inf = float("nan"), float("inf")
    p = zr.positions([(nan, inf), (-inf, 1e9), (-1e9, 40000.7), (-32768.5, 32767.9), (0.99, -0.99), (-32767.9, 32766.9), (-1.5, 1.5)])
    assert p.tolist() == [[-32768, 32767], [-32768, 32767], [-32768, 32767], [-32768, 32767], [0, 0], [-32767, 32766], [-1, 1]]


def run(case, batch=3):
    return ze.reference_steps(case, batch)


def reject_positions(stream):
    old, _, st, kp = stream
    return zr.positions(old[(st == 1) & (kp == 0)])


@pytest.mark.parametrize("h,w", [(48, 64), (480, 640)])
def test_clamp_case_lands_on_both_ends_of_both_axes(h, w):
    case = ze.clamp(h, w)
    pos = reject_positions(case["steps"][0][0])
    for axis in (0, 1):
        assert {-32768, 32767} <= set(pos[:, axis].tolist())
    assert [0, 0] in pos.tolist()                                # -0.9 truncates toward zero
    out = run(case)
    t0, m0 = out[0][0]
    assert t0.stats[1] == 3 and t0.stats[4] == 13 and sorted(t0.zones[:3, 3].tolist()) == [-32768, -20010, -5]     # smallest x of each zone
    assert not m0[0, 0] and m0[h - 1, w - 1]                     # the zone across the origin is in the mask
    assert out[1][0][0].stats[2] == 3 and out[1][0][0].stats[5] == 9 and out[1][1][0].stats[5] == 0
    assert out[0][1][0].stats[1] == 2 and out[0][1][0].zones[0, 3:9].tolist() == [-32768, 100, -32765, 108, -32768, 104]


def guard_pairs(case, monkeypatch):
    """Runs the case on the reference and counts the (pixel, edge) pairs of every call of rule 5 whose |cross| exceeds 2^25."""
    count = [0]
    inside = zr.inside

    def counting(px, py, V, r):
        px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
        n = len(V)
        for i in range(0 if n == 0 else 1 if n <= 2 else n):
            (ax, ay), (bx, by) = V[i], V[(i + 1) % n]
            count[0] += int(np.count_nonzero(np.abs((int(bx) - int(ax)) * (py - int(ay)) - (int(by) - int(ay)) * (px - int(ax))) > 1 << 25))
        return inside(px, py, V, r)
    monkeypatch.setattr(zr, "inside", counting)
    out = run(case)
    monkeypatch.setattr(zr, "inside", inside)
    return out, count[0]


def test_far_case_passes_the_guard_saturates_and_expires(monkeypatch):
    out, guarded = guard_pairs(ze.far("plain"), monkeypatch)
    print("(reject, edge) pairs with |cross| above 2^25:", guarded)
    assert guarded > 0
    offs = [out[k][0][0].motion[0, :2].tolist() for k in range(5)]
    assert offs == [[3e5 * (k + 1), -2e5 * (k + 1)] for k in range(5)] and abs(offs[3][0]) > 1 << 20 > abs(offs[2][0])     # saturated from the fourth step on
    assert out[0][0][0].zones[0, :3].tolist() == [5, 3, 4] and out[4][0][0].zones[0, 0] == 1 and not out[5][0][0].zones.any()
    assert all(out[k][0][0].stats[4] == 5 and out[k][0][0].stats[5] == 0 for k in range(1, 6))


def test_far_case_without_a_number(monkeypatch):
    out, guarded = guard_pairs(ze.far("nan"), monkeypatch)
    assert guarded > 0
    flow = out[0][0][0].motion[0, 2:]
    assert np.isnan(flow[0]) and flow[1] == np.inf
    t = out[1][0][0]
    assert np.isnan(t.motion[0, 0]) and t.motion[0, 1] == np.inf and zr.shifted(out[0][0][0], 0)[0].tolist() == [300 - (1 << 20), 200 + (1 << 20)]


def test_drift_case_meets_half_integers_and_is_refreshed_there():
    out = run(ze.drift_negative())
    offs = [out[k][0][0].motion[0, :2].tolist() for k in range(5)]
    assert offs == [[-9000.5, 7000.5], [-18001.0, 14001.0], [-27001.5, 21001.5], [-36002.0, 28002.0], [-45002.5, 35002.5]]
    assert [out[k][0][0].stats[[2, 5]].tolist() for k in range(5)] == [[0, 0], [1, 1], [0, 0], [1, 1], [0, 0]]
    assert out[4][0][0].stats[0] == 1                            # still live when the last reject misses it
    t = out[3][0][0].copy()                                      # the table step 5 meets; with the offset held at -32768 that reject is inside
    t.motion[0, 0] = -32768
    p = reject_positions(ze.drift_negative()["steps"][4][0])
    assert zr.inside(p[:, 0], p[:, 1], zr.shifted(t, 0), 12).all()


def test_hull_cases_have_32_33_and_34_vertices():
    case = ze.hulls()
    assert [len(zr.hull(zr.positions(p))) for p in case["polys"]] == [32, 33, 34]
    out = run(case)
    tabs = [out[0][b][0] for b in range(3)]
    assert [int(t.zones[0, 1]) for t in tabs] == [32, 4, 4] and [int(t.zones[0, 2]) for t in tabs] == [32, 33, 34]
    assert all(t.stats[1] == 1 and t.stats[4] == t.zones[0, 2] for t in tabs)
    print("label sweeps:", [int(t.stats[6]) for t in tabs])
    assert tabs[1].zones[0, 3:11].tolist() == [292, 100, 308, 100, 308, 300, 292, 300]
    assert not any(out[1][b][0].zones.any() for b in range(3))


def test_setting_extremes():
    out = run(ze.singletons())
    for b in (0, 1):
        t, mask = out[0][b]
        assert t.stats.tolist()[:5] == [0, 20, 0, 4, 20] and not t.zones.any() and np.count_nonzero(mask == 0) == 16
    assert out[0][0][1][85, 110] == 0 and out[0][0][1][10, 10] == 1      # slot 0 went to the last insert, the first is gone
    out = run(ze.duplicates())
    for b in (0, 1):
        assert out[0][b][0].stats.tolist()[:5] == [16, 20, 0, 4, 43] and (out[0][b][0].zones[:, 1:3] == [1, 2]).all()
    out = run(ze.one_slot())
    assert out[0][0][0].stats.tolist()[:4] == [1, 3, 0, 2] and out[0][0][0].zones[0, 3:5].tolist() == [20, 35] and not out[0][0][0].zones[1:].any()
    assert out[1][0][0].stats.tolist()[:4] == [1, 1, 0, 1] and out[1][0][0].zones[0, 3:5].tolist() == [45, 30] and out[1][1][0].zones[0, :5].tolist() == [1, 3, 3, 10, 10]
    out = run(ze.link_4096())
    assert [[int(out[k][b][0].stats[1]) for b in range(3)] for k in (0, 1)] == [[1, 2, 1], [2, 1, 1]]
    assert all(out[k][b][0].stats[5] == 0 and not out[k][b][0].zones.any() for k in (0, 1) for b in range(3))
    out = run(ze.radius_0())
    assert [int(out[0][b][0].zones[0, 1]) for b in range(3)] == [1, 2, 2]
    assert [np.argwhere(out[0][b][1] == 0).tolist() for b in range(3)] == [[[30, 20]]] + [[[10, 10], [13, 17], [16, 24], [19, 31], [22, 38]]] * 2


def test_span_case_takes_products_past_32_bits():
    case = ze.span()
    out = run(case)
    for b in (0, 1):
        t, mask = out[0][b]
        assert t.stats[1] == 1 and t.zones[0, 1:9].tolist() == [3, 35, -32768, -32768, 32767, -32768, 0, 32767] and not mask.any()
    V = zr.shifted(out[0][0][0].copy(), 0) - np.rint(out[0][0][0].motion[0, :2]).astype(np.int64)      # as drawn in step 1: offset 0
    ex = int(V[1, 0] - V[0, 0])
    assert ex == 65535 and ex * (1 - int(V[0, 1])) >= 1 << 31    # from row 1 on, (b - a).x (p - a).y leaves 32 bits
    assert out[1][0][0].stats[5] == 3 and out[1][0][0].stats[2] == 1     # of the probes (0, 0) is inside and two land on the vertex (32767, -32768)


def test_flag_bytes_case_rejects_only_status_1_keep_0():
    case = ze.flag_bytes()
    old, new, st, kp = case["steps"][0][0]
    assert len(old) == 512 and all(np.count_nonzero((st == a) & (kp == q)) == 32 for a in ze.BYTES for q in ze.BYTES)
    out = run(case)
    assert [int(out[0][b][0].stats[4]) for b in range(3)] == [32, 32, 0] and [int(out[0][b][0].stats[1]) for b in range(3)] == [1, 1, 0]
    assert out[0][0][0].zones[0, 2] == 32 and out[0][1][0].zones[0, 2] == 32


@pytest.mark.parametrize("h,w", [(33, 47), (17, 65), (16, 64)])
@pytest.mark.parametrize("radius", [0, 20])
def test_tiling_cases_cross_every_border_and_corner(h, w, radius):
    assert h % 16 or w % 64 or (h, w) == (16, 64)
    case = ze.tiling(h, w, radius, "big")
    out = run(case)
    t, mask = out[0][0]
    v = t.zones[0, 3:9].reshape(3, 2)
    assert t.stats[1] == 1 and v[:, 0].min() < 0 and v[:, 0].max() >= w and v[:, 1].min() < 0 and v[:, 1].max() >= h
    assert case["masks"][0][0].any() and not mask.any()          # the image lies inside it, corners included
    case = ze.tiling(h, w, radius, "small")
    out = run(case)
    for b in (1, 2):
        t = out[0][b][0]
        assert t.stats[1] == 4 and (t.zones[:4, 1] == 3).all()
        for z in range(4):
            v = t.zones[z, 3:9].reshape(3, 2)
            inx, iny = (v[:, 0] >= 0) & (v[:, 0] < w), (v[:, 1] >= 0) & (v[:, 1] < h)
            assert (inx & iny).any() and not (inx & iny).all(), (b, z, v)
    for k in range(4):                                           # zeros of mask_in survive, ones outside every zone too
        for b in range(3):
            assert not out[k][b][1][case["masks"][k][b] == 0].any()
    offs = [out[k][1][0].motion[0, :2].tolist() for k in range(3)]
    assert offs == [[-0.5, 2.5], [-1.0, 5.0], [-1.5, 7.5]] and out[2][2][0].motion[0, :2].tolist() == [4.5, -1.5]


def test_big_count_case():
    case = ze.big_count()
    (old0, _, st0, kp0), (old1, _, st1, kp1) = case["steps"][0]
    rej = np.nonzero((st0 == 1) & (kp0 == 0))[0]
    assert len(old0) == len(old1) == 4096 and len(rej) == 1200 and rej.min() >= 2800 and ((st1 == 1) & (kp1 == 0)).all()
    lab, _ = zr.labels(zr.positions(old0[rej]), case["setting"]["link"])
    sizes = np.bincount(lab)
    assert (sizes[lab[rej > 4000]] >= 3).any()                   # a member of a zone with a point index above 4000
    assert len(set(sizes[sizes > 0].tolist())) >= 4 and np.count_nonzero(sizes >= 3) > 16        # mixed sizes, more clusters than slots
    out = run(case, 2)
    s0, s1 = out[0][0][0].stats, out[0][1][0].stats
    assert s0[4] == 1200 and s0[4] - s0[5] > 1024 and s0[1] > 16 and s0[0] == 16
    assert s1.tolist()[:6] == [16, 16, 0, 0, 4096, 0]
    assert out[1][1][0].stats.tolist()[:6] == [16, 0, 16, 0, 4096, 4096] and 0 < out[1][0][0].stats[5] < 1200
    print("label sweeps:", [[int(out[k][b][0].stats[6]) for b in (0, 1)] for k in (0, 1)])
