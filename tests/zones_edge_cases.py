"""Exclusion zones at the limits of their rules: the step runner of the zone tests and the edge cases as data.  No test file.

run_steps drives ofk_zones_step and tests/zones_reference.py side by side and compares mask, table, motion bits and statistics behind
every step.  A case is dict(setting, h, w, steps[, masks]): steps[k][b] = (old, new, status, keep) of stream b in step k, masks
[steps, B, h, w] u8 or absent.  Each case is stated once, here; tests/test_zones_edge_cases.py asserts on the reference alone the
condition that makes it a test of its edge, tests/test_gpu_zones_edges.py runs it on the device."""
import functools

import numpy as np

import zones_reference as zr
from point_stage_helpers import bits


def rejects(pts, flow=(0.0, 0.0)):
    """One stream's step from reject positions: (old, new, status, keep)."""
    old = np.asarray(pts, np.float32).reshape(-1, 2)
    return old, old + np.asarray(flow, np.float32), np.ones(len(old), np.uint8), np.zeros(len(old), np.uint8)


NONE = rejects(np.zeros((0, 2)))


def padded(streams, batch):
    return list(streams) + [NONE] * (batch - len(streams))


def reference_steps(case, batch):
    """The reference alone: per step and stream (table behind the step, mask), for the conditions of the CPU tests."""
    s = dict(zr.DEFAULT, **case["setting"])
    tables = [zr.Table() for _ in range(batch)]
    out = []
    for k, streams in enumerate(case["steps"]):
        row = []
        for b, (o, n, a, q) in enumerate(padded(streams, batch)):
            mask = zr.step(tables[b], s, o, n, a, q, case["h"], case["w"], None if case.get("masks") is None else case["masks"][k][b])
            row.append((tables[b].copy(), mask))
        out.append(row)
    return out


def run_steps(ctx, setting, steps, h, w, masks=None, batch=None, stride=None):
    """steps: per step a list of at most `batch` streams' (old, new, status, keep), laid out at `stride` points per stream (None: the
    context's limits).  Compares mask, table and statistics behind every step and returns the reference tables and the last masks."""
    B, S = ctx.max_batch if batch is None else batch, ctx.max_pts if stride is None else stride
    s = dict(zr.DEFAULT, **setting)
    ctx.set_zones(**s)
    ctx.zones_reset()
    tables = [zr.Table() for _ in range(B)]
    mask = None
    for k, streams in enumerate(steps):
        streams = padded(streams, B)
        old = np.zeros((B, S, 2), np.float32); new = np.zeros((B, S, 2), np.float32)
        st = np.zeros((B, S), np.uint8); kp = np.ones((B, S), np.uint8); counts = np.zeros(B, np.int32)
        for b, (o, n, a, q) in enumerate(streams):
            m = len(o)
            old[b, :m], new[b, :m], st[b, :m], kp[b, :m], counts[b] = o, n, a, q, m
            old[b, m:] = 7.0; st[b, m:] = 1; kp[b, m:] = 0       # behind the count: never read
        mask_in = None if masks is None else masks[k]
        mask = ctx.zones_step(old, new, st, kp, counts, h, w, mask_in)
        got = ctx.zones_download(B)
        for b, (o, n, a, q) in enumerate(streams):
            ref = zr.step(tables[b], s, o, n, a, q, h, w, None if mask_in is None else mask_in[b])
            tag = (k, b)
            assert np.array_equal(got["stats"][b], tables[b].stats), (tag, got["stats"][b], tables[b].stats)
            assert np.array_equal(got["zones"][b], tables[b].zones), (tag, got["zones"][b][:, :12], tables[b].zones[:, :12])
            assert np.array_equal(bits(got["motion"][b]), bits(tables[b].motion)), (tag, got["motion"][b], tables[b].motion)
            assert np.array_equal(mask[b], ref), (tag, int(np.count_nonzero(mask[b] != ref)))
    return tables, mask


def run_case(ctx, case, **kw):
    return run_steps(ctx, case["setting"], case["steps"], case["h"], case["w"], case.get("masks"), **kw)


NAN, INF = float("nan"), float("inf")
# rule 1's limits: beyond both ends of the 16-bit range, not a number, infinities, fractions that truncate toward zero.  No three of
# their positions link at link 70: they form no zone of three members.
PROBES = [(1e9, -1e9), (NAN, 5.0), (-40000.0, 40000.0), (-0.9, -0.9), (INF, -INF)]
QUAD = [(300, 200), (360, 200), (420, 200), (360, 260)]         # three vertices, four members; the rightmost vertex is (420, 200)


@functools.lru_cache(None)
def clamp(h, w):
    """Positions at and beyond the 16-bit range.  A zone on the clamp line (positions (-32768, 100), (-32768, 104), (-32765, 108)),
    one built, sorted and stored from negative coordinates near (-20000, 30000), one across the image's origin from fractions that
    truncate toward zero; the second step's rejects fall back into them."""
    line = [(-32768.5 - 3, 100.2), (-32768.5, 104.9), (-32768.5 + 3, 108.5)]
    neg = [(-20000.3, 30000.7), (-19990.9, 30010.2), (-20010.5, 29995.5)]
    org = [(-5.5, 3.2), (4.7, -6.9)]                             # with the probe at (-0.9, -0.9): (0, 0), (-5, 3), (4, -6)
    one = rejects(PROBES + line + neg + org, (1.5, -0.25))
    return dict(setting=dict(link=70, min_members=3, radius=12, ttl=4), h=h, w=w, steps=[[one, rejects(line + neg)], [one, rejects(PROBES)], [NONE, NONE]])


@functools.lru_cache(None)
def far(variant):
    """The quad drifts by (3e5, -2e5) a step: the offset saturates at +-2^20 from the fourth step on, |cross| passes 2^25 against the
    probes.  variant "nan": one member's new position is (NaN, inf), so the flow is, and the offset reads -2^20 / +2^20 at once."""
    old, new, st, kp = rejects(QUAD, (3e5, -2e5))
    if variant == "nan":
        new = new.copy(); new[2] = NAN, INF
    return dict(setting=dict(link=70, min_members=3, radius=12, ttl=6), h=48, w=64, steps=[[(old, new, st, kp)]] + [[rejects(PROBES)]] * 5)


@functools.lru_cache(None)
def drift_negative():
    """The quad drifts by (-9000.5, 7000.5) a step: offsets (-9000.5, 7000.5), (-18001, 14001), (-27001.5, 21001.5), (-36002, 28002) -
    half-integers of both parities.  Step 2: a reject exactly `radius` right of the rightmost vertex where half-to-even puts it
    ((420 - 9000, 200 + 7000); rounding half away from zero puts it a pixel further left and down).  Step 4: a reject inside the
    triangle.  Step 5: a reject where the zone would stand were its offset held at -32768; at -36002 no position reaches it."""
    r = 12
    steps = [[rejects(QUAD, (-9000.5, 7000.5))], [rejects([(420 - 9000 + r - 0.5, 200 + 7000 + 0.5)])], [NONE], [rejects([(-26638.5, 21216.5)])],
             [rejects([(360 - 32768 - 0.5, 220 + 28002 + 0.5)])]]
    return dict(setting=dict(link=70, min_members=3, radius=r, ttl=6), h=48, w=64, steps=steps)


def polygon(upper_from, upper_to):
    lower = [(k, k * k) for k in range(-8, 9)]
    upper = [(k, 200 - k * k) for k in range(upper_from, upper_to + 1)]
    return np.array(lower + upper, np.float32) + np.float32([300, 100])


@functools.lru_cache(None)
def hulls():
    """Hulls of 32, 33 and 34 vertices, one per stream, in shuffled index order: the first is kept, the others become their box."""
    rng = np.random.default_rng(32)
    polys = [polygon(-7, 7), polygon(-7, 8), polygon(-8, 8)]
    streams = [rejects(p[rng.permutation(len(p))] + np.float32(0.25), (0.5, -2.5)) for p in polys]
    return dict(setting=dict(link=100, min_members=3, radius=5, ttl=2), h=480, w=640, steps=[streams, [NONE] * 3], polys=polys)


GRID20 = np.array([(10 + 25 * i, 10 + 25 * j) for j in range(4) for i in range(5)], np.float32)


@functools.lru_cache(None)
def singletons():
    """20 single rejects, 16 slots, every limit of the setting at its lowest: a zone inserted in the step is evicted in it (equal ttl:
    inserts 17 to 20 all take slot 0), drawn in its mask and freed by rule 7 in the same step."""
    return dict(setting=dict(link=1, min_members=1, radius=0, ttl=1, max_zones=16), h=96, w=120, steps=[[rejects(GRID20), rejects(GRID20[::-1] + np.float32(0.9))]])


@functools.lru_cache(None)
def duplicates():
    """link 1 links identical truncated positions only: each grid point and its +0.75 copy are a zone, the neighbours a pixel away none."""
    near = GRID20[[0, 7, 19]] + np.float32([[1, 0], [0, 1], [-1, -1]])
    p = np.concatenate([GRID20, near, GRID20 + np.float32(0.75)])
    return dict(setting=dict(link=1, min_members=2, radius=0, ttl=2, max_zones=16), h=96, w=120, steps=[[rejects(p, (1.0, 0.5)), rejects(p[::-1])], [NONE, NONE]])


TRI = np.array([[0, 0], [6, 3], [2, 7]], np.float32)


@functools.lru_cache(None)
def one_slot():
    """max_zones 1: three clusters in a step, each evicts the one before; the next step's cluster evicts the last."""
    a = np.concatenate([TRI + np.float32(o) for o in ([10, 10], [40, 12], [20, 35])])
    return dict(setting=dict(link=10, min_members=3, radius=3, ttl=3, max_zones=1), h=48, w=64, steps=[[rejects(a, (0.5, 0.5)), rejects(a[:3])], [rejects(TRI + np.float32([45, 30])), NONE]])


@functools.lru_cache(None)
def link_4096():
    """link 4096, outside the image: two clusters whose nearest members are 4095 apart on one axis are one zone, 4096 apart two.
    ttl 1, so the second step (the other axis) starts from an empty table."""
    def pair(axis, gap):
        shift = np.zeros(2, np.float32); shift[axis] = 6 + gap   # TRI spans 0..6 in x and 0..7 in y
        if axis == 1:
            shift[axis] += 1
        return rejects(np.concatenate([TRI + np.float32([1000, 2000]), TRI + np.float32([1000, 2000]) + shift]), (-2.5, 1.5))
    return dict(setting=dict(link=4096, min_members=3, radius=7, ttl=1), h=48, w=64, steps=[[pair(0, 4095), pair(0, 4096), pair(1, 4095)], [pair(1, 4096), pair(1, 4095), pair(0, 4095)]])


@functools.lru_cache(None)
def span():
    """One zone over the whole 16-bit range: chains of rejects 4095 apart (link 4096) along y = -32768 and up x = 0 make the triangle
    (-32768, -32768), (32767, -32768), (0, 32767) with the image inside it.  An edge is 65535 long and every pixel is more than 32768
    from it: edge times distance passes 2^31, the cross products 2^32, and only the sign test of rule 5 (a) decides."""
    xs = list(range(-32768, 32767, 4095)) + [32767]
    ys = list(range(-32768, 32767, 4095)) + [32767]
    p = [(float(x), -32768.0) for x in xs] + [(0.5, float(y)) for y in ys[1:]]
    p[0] = (-1e9, -1e9); p[len(xs) - 1] = (1e9, -40000.0); p[-1] = (0.9, 1e9)      # the three vertices come from beyond the range
    return dict(setting=dict(link=4096, min_members=3, radius=0, ttl=2), h=48, w=64, steps=[[rejects(p, (0.25, 0.25)), rejects(p[::-1])], [rejects(PROBES), NONE]])


@functools.lru_cache(None)
def radius_0():
    """radius 0: a one-vertex zone is its pixel, a two-vertex zone the lattice points of its segment (slope 3/7)."""
    return dict(setting=dict(link=30, min_members=3, radius=0, ttl=2), h=48, w=64, steps=[[rejects([(20.5, 30.5)] * 3), rejects([(10, 10), (24, 16), (38, 22)]), rejects([(10, 10), (38, 22), (10, 10)])], [NONE] * 3])


BYTES = (0, 1, 2, 255)


@functools.lru_cache(None)
def flag_bytes():
    """Every (status, keep) of {0, 1, 2, 255}^2 on 32 points each, 512 in all (the count equals the stride), all inside one link
    distance: only status == 1 with keep == 0 rejects."""
    rng = np.random.default_rng(255)
    st = np.repeat(np.array([a for a in BYTES for _ in BYTES], np.uint8), 32)
    kp = np.repeat(np.array([q for _ in BYTES for q in BYTES], np.uint8), 32)
    perm = rng.permutation(512)
    st, kp = st[perm], kp[perm]
    old = np.stack([rng.uniform(10, 50, 512), rng.uniform(8, 40, 512)], 1).astype(np.float32)
    new = old + rng.normal(0, 2, old.shape).astype(np.float32)
    return dict(setting=dict(link=48, min_members=3, radius=2, ttl=3), h=48, w=64, steps=[[(old, new, st, kp), (old, new, kp, st), (old, new, st, st)]])


@functools.lru_cache(None)
def tiling(h, w, radius, which):
    """Masks that are no multiple of the 64 x 16 tile, mask_in with random zeros.  which "big": a zone larger than the image, all
    four corners clipped (link 4096).  which "small": four zones across one border each in stream 1, four across one corner each in
    stream 2 (link 5: their nearest members are at least 11 apart).  The flows are half-integers of both parities and signs, so the
    three later steps draw every zone where half-to-even puts it."""
    rng = np.random.default_rng(h * 1000 + w)
    masks = (rng.random((4, 3, h, w)) < 0.9).astype(np.uint8)
    if which == "big":
        streams, link = [rejects([(-30.5, -20.5), (w + 40.5, -25.5), (w // 2 + 0.5, h + 60.5)], (0.5, -1.5))], 4096
    else:
        small = np.array([[-2, -2], [2, -1], [0, 2]], np.float32)
        border = rejects(np.concatenate([small + np.float32(c) for c in ((0, h // 2), (w - 1, h // 2), (w // 2, 0), (w // 2, h - 1))]), (-0.5, 2.5))
        corner = rejects(np.concatenate([small + np.float32(c) for c in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1))]), (1.5, -0.5))
        streams, link = [NONE, border, corner], 5
    return dict(setting=dict(link=link, min_members=3, radius=radius, ttl=5), h=h, w=w, steps=[streams] + [[NONE] * 3] * 3, masks=masks)


CLUSTERS16 = np.array([(80 + 150 * i, 60 + 110 * j) for j in range(4) for i in range(4)], np.float32)


@functools.lru_cache(None)
def big_count():
    """4096 points per stream, the count equal to the stride.  Stream 0: 1200 rejects, all at indices >= 2800, on a jittered grid at
    link 12 (components of mixed size), the rest kept.  Stream 1: every point a reject, in 16 clusters of 256 on 8 x 8 pixels each;
    the second step's rejects all fall into the first step's zones."""
    rng = np.random.default_rng(4096)
    n = 4096
    gx, gy = np.meshgrid(np.arange(64), np.arange(64))
    old0 = (np.stack([gx.ravel() * 9.5 + 15, gy.ravel() * 7 + 12], 1) + rng.uniform(-4, 4, (n, 2))).astype(np.float32)[rng.permutation(n)]
    st0 = np.ones(n, np.uint8); kp0 = np.ones(n, np.uint8)
    kp0[2800 + rng.permutation(n - 2800)[:1200]] = 0
    new0 = old0 + rng.normal(0, 1.5, (n, 2)).astype(np.float32)
    old1 = (np.repeat(CLUSTERS16, 256, 0) + rng.uniform(0, 8, (n, 2)).astype(np.float32))[rng.permutation(n)]
    new1 = old1 + np.float32([0.5, -0.25])
    one = np.ones(n, np.uint8); zero = np.zeros(n, np.uint8)
    streams = [(old0, new0, st0, kp0), (old1, new1, one, zero)]
    return dict(setting=dict(link=12, min_members=3, radius=20, ttl=3), h=480, w=640, steps=[streams, streams])
