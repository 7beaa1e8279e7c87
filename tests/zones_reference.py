"""Exclusion zones (include/ofk.h: ofk_zones) restated in numpy: the reference the zone tests compare the device against bit for bit,
and the constructor of a NodeLoop whose re-detection mask carries the zones.  All image arithmetic is Python / int64 integers, the two float steps (the
mean flow, the advection) are written in the precision the header states.  Test infrastructure only.

What the zones achieve is stated on this loop (tests/test_zones_reference.py): robust_stream_oracle.sequence at 480 x 640, 12 frames,
max_corners 200, min_features 199, mask radius 15, the robust solve with drop; zones at their defaults (link 48, 3 members, radius 20,
ttl 30, 16 zones).  Measured with the committed code, seeds 900 and 901, without -> with zones:
    points dropped over the 11 steps                        174 -> 97         207 -> 103
    share of the tracks on the object behind a re-detection,
    largest of all steps                                    0.087 -> 0.041    0.104 -> 0.021
    largest from the third step on                          0.057 -> 0.015    0.104 -> 0.021
    tracks after a step                                     170..197          167..197 (unchanged by the zones)
    relative velocity error, largest                        0.0050 -> 0.0050  0.0048 -> 0.0048"""
import numpy as np

from stream_oracle import NodeLoop

OFF, HULL = 0, 1
ZONE_MAX, ZONE_VERTS = 16, 32
ZONE_INTS = 3 + 2 * ZONE_VERTS                                   # ttl, vertices, members, the vertices (x, y)
ZONE_FLOATS = 4                                                  # off x, y; flow x, y
ZONE_STATS = 8                                                   # live, inserted, refreshed, evicted, rejects, absorbed, label sweeps, reserved
POS_LIM, OFF_LIM = 32767, 1 << 20
DEFAULT = dict(link=48, min_members=3, radius=20, ttl=30, max_zones=16)


class Table:
    """One stream's table: zones [16][ZONE_INTS] i32, motion [16][4] f32, stats [ZONE_STATS] i32 of the latest step."""

    def __init__(self):
        self.zones = np.zeros((ZONE_MAX, ZONE_INTS), np.int32)
        self.motion = np.zeros((ZONE_MAX, ZONE_FLOATS), np.float32)
        self.stats = np.zeros(ZONE_STATS, np.int32)

    def copy(self):
        t = Table()
        t.zones, t.motion, t.stats = self.zones.copy(), self.motion.copy(), self.stats.copy()
        return t

    def live(self):
        return [z for z in range(ZONE_MAX) if self.zones[z, 0] > 0]


def positions(pts):
    """Truncated positions, each axis first brought into -32768..32767 (not a number: -32768)."""
    p = np.asarray(pts, np.float32).reshape(-1, 2)
    p = np.where(np.isnan(p), np.float32(-POS_LIM - 1), np.clip(p, np.float32(-POS_LIM - 1), np.float32(POS_LIM)))
    return np.trunc(p).astype(np.int64)


def hull(pts):
    """Andrew's chain on integer points: duplicates merged, collinear points removed, lower then upper (of_library._hull)."""
    P = sorted(set((int(x), int(y)) for x, y in pts))
    if len(P) <= 2:
        return P

    def half(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and (out[-1][0] - out[-2][0]) * (p[1] - out[-2][1]) - (out[-1][1] - out[-2][1]) * (p[0] - out[-2][0]) <= 0:
                out.pop()
            out.append(p)
        return out
    lo, up = half(P), half(P[::-1])
    return lo[:-1] + up[:-1]


def zone_vertices(pts):
    """Rule 4: the hull, or the bounding box when it has more than 32 vertices."""
    v = hull(pts)
    if len(v) > ZONE_VERTS:
        xs, ys = [p[0] for p in v], [p[1] for p in v]
        x0, x1, y0, y1 = min(xs), max(xs), min(ys), max(ys)
        v = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    return v


def shifted(table, z):
    """Rule 5's V: the zone's vertices plus rint(off), half to even, each axis brought into +-2^20 (not a number: -2^20)."""
    n = int(table.zones[z, 1])
    v = table.zones[z, 3:3 + 2 * n].astype(np.int64).reshape(n, 2)
    o = np.rint(table.motion[z, :2])
    o = np.where(np.isnan(o), np.float32(-OFF_LIM), np.clip(o, np.float32(-OFF_LIM), np.float32(OFF_LIM))).astype(np.int64)
    return v + o


def inside(px, py, V, r):
    """Rule 5 for arrays of pixels.  cross^2 <= r^2 L is only formed where |cross| <= 2^25, so that the square stays inside int64; beyond,
    it is false anyway: a hull's vertices lie within -32768..32767 per axis, so L <= 2^33 and r^2 L < 2^49 < 2^50 (r <= 255)."""
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    n = len(V)
    res = np.zeros(px.shape, bool)
    if n == 0:
        return res
    conv = np.ones(px.shape, bool)
    r2 = int(r) * int(r)
    for i in range(1 if n <= 2 else n):
        ax, ay = int(V[i][0]), int(V[i][1]); bx, by = int(V[(i + 1) % n][0]), int(V[(i + 1) % n][1])
        ex, ey, qx, qy = bx - ax, by - ay, px - ax, py - ay
        cr = ex * qy - ey * qx
        conv &= cr >= 0
        t, L = qx * ex + qy * ey, ex * ex + ey * ey
        near = np.abs(cr) <= (1 << 25)
        res |= (qx * qx + qy * qy <= r2) | ((px - bx) ** 2 + (py - by) ** 2 <= r2) | ((t > 0) & (t < L) & near & (np.where(near, cr, 0) ** 2 <= r2 * L))
    if n >= 3:
        res |= conv
    return res


def labels(pos, link):
    """Rule 3 as the device computes it: min-label hooking of the roots, then full pointer jumping, until no root hooks.
    -> (label = smallest member index per point, sweeps)."""
    m = len(pos)
    lab = np.arange(m)
    if m == 0:
        return lab, 0
    d = np.abs(pos[:, None, :] - pos[None, :, :])
    nb = (d[..., 0] < link) & (d[..., 1] < link)
    sweeps = 0
    while True:
        sweeps += 1
        mj = np.where(nb, lab[None, :], m).min(1)
        hook = np.arange(m)
        np.minimum.at(hook, lab, mj)
        roots = lab == np.arange(m)
        if not (hook[roots] < np.arange(m)[roots]).any():
            return lab, sweeps
        lab = np.where(roots, hook, lab)
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt


def update(table, s, old, new, status, keep):
    """Rules 1-4 on one stream's points.  s: dict(link, min_members, radius, ttl, max_zones)."""
    old = np.asarray(old, np.float32).reshape(-1, 2); new = np.asarray(new, np.float32).reshape(-1, 2)
    rej = np.nonzero((np.asarray(status).ravel() == 1) & (np.asarray(keep).ravel() == 0))[0]
    pos = positions(old[rej])
    st = np.zeros(ZONE_STATS, np.int32)
    st[4] = len(rej)
    absorbed = np.zeros(len(rej), bool)
    for z in table.live():                                       # rule 2
        hit = inside(pos[:, 0], pos[:, 1], shifted(table, z), s["radius"]) if len(rej) else np.zeros(0, bool)
        if hit.any():
            table.zones[z, 0] = s["ttl"]; st[2] += 1
        absorbed |= hit
    st[5] = int(absorbed.sum())
    rej, pos = rej[~absorbed], pos[~absorbed]
    lab, st[6] = labels(pos, s["link"])                          # rule 3
    for root in sorted(set(lab.tolist())):                       # rule 4
        mem = np.nonzero(lab == root)[0]
        if len(mem) < s["min_members"]:
            continue
        free = [z for z in range(s["max_zones"]) if table.zones[z, 0] == 0]
        if free:
            z = free[0]
        else:
            z = min(range(s["max_zones"]), key=lambda k: (table.zones[k, 0], k)); st[3] += 1
        v = zone_vertices(pos[mem])
        fx = fy = 0.0
        for i in rej[mem]:
            fx += float(new[i, 0]) - float(old[i, 0]); fy += float(new[i, 1]) - float(old[i, 1])
        table.zones[z] = 0
        table.zones[z, :3] = s["ttl"], len(v), len(mem)
        table.zones[z, 3:3 + 2 * len(v)] = np.array(v, np.int64).ravel()
        table.motion[z] = 0.0, 0.0, np.float32(fx / len(mem)), np.float32(fy / len(mem))
        st[1] += 1
    table.stats = st


def render(table, s, mask):
    """Rule 6: zero every live zone's pixels in mask [h, w] u8, in place."""
    h, w = mask.shape
    for z in table.live():
        V = shifted(table, z)
        r = s["radius"]
        x0, x1 = max(0, int(V[:, 0].min()) - r), min(w - 1, int(V[:, 0].max()) + r)
        y0, y1 = max(0, int(V[:, 1].min()) - r), min(h - 1, int(V[:, 1].max()) + r)
        if x0 > x1 or y0 > y1:
            continue
        yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        mask[y0:y1 + 1, x0:x1 + 1][inside(xx, yy, V, r)] = 0
    return mask


def age(table):
    """Rule 7."""
    for z in table.live():
        table.motion[z, :2] = table.motion[z, :2] + table.motion[z, 2:]          # f32
        table.zones[z, 0] -= 1
        if table.zones[z, 0] == 0:
            table.zones[z] = 0; table.motion[z] = 0
    table.stats[0] = len(table.live())


def step(table, s, old, new, status, keep, h, w, mask_in=None):
    """ofk_zones_step for one stream: rules 1-7, -> the mask of rule 6."""
    update(table, s, old, new, status, keep)
    mask = np.ones((h, w), np.uint8) if mask_in is None else np.array(mask_in, np.uint8)
    render(table, s, mask)
    age(table)
    return mask


class ZoneNodeLoop(NodeLoop):
    """NodeLoop with the zone table of one stream (stream_oracle.NodeLoop's zones= and replace=): the step's rejects (tracked, not kept
    by the solver) update the table, an append-mode re-detection runs behind the disc mask with the zones zeroed in it, a
    replace-mode one behind a mask of the zones alone, then the zones move on and age."""

    def __init__(self, first_frame, cfg, min_feat, radius, setting=None, replace=False, **kw):
        super().__init__(first_frame, cfg, min_feat, radius, zones=dict(setting or {}), replace=replace, **kw)
