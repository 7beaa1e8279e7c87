"""Test-side restatement of the track table (include/ofk.h: ofk_set_track_table) and the experiment its seed is held to.

begin / replace / update / seed_points   rules 1-3, 5 and 6 of ofk.h in numpy for ONE stream, float32 where the rules say float32.  A
             table is a dict of arrays of `stride` rows (ids u32, age, birth_step i32, birth_xy, flow_xy [S,2] f32) plus the ints
             step, next_id and count; rows at and beyond count keep whatever they held, as on the device.
experiment   the ramp experiment of the track-table issue: three motions, 640 x 480, 300 corners, window 15, the motion ramping
             from 10 % to 100 % over ten frames and holding for two, no re-detection; plain maxLevel 3 against LK seeded with each
             track's last flow at maxLevel 1 (and 0), and the two conditions every implementation is held to.
"""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
for _p in (ROOT, _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import lk_seed_reference as lsr  # noqa: E402
from oracle import image_oracle as io  # noqa: E402

F32 = np.float32
STATS = 8


def empty(stride):
    return dict(ids=np.zeros(stride, np.uint32), age=np.zeros(stride, np.int32), birth_step=np.zeros(stride, np.int32),
                birth_xy=np.zeros((stride, 2), F32), flow_xy=np.zeros((stride, 2), F32), step=0, next_id=0, count=0)


def copy(t):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in t.items()}


def begin(pts, n, stride=None):
    """Rule 1: the table of n freshly detected tracks pts [>= n, 2] -> (table, stats)."""
    pts = np.asarray(pts, F32).reshape(-1, 2)
    t = empty(len(pts) if stride is None else stride)
    t["ids"][:n] = np.arange(n, dtype=np.uint32)
    t["birth_xy"][:n] = pts[:n]
    t["next_id"] = t["count"] = int(n)
    return t, np.array([n, 0, 0, n, 0, 0, n, 0], np.int32)


def replace(t, new_pts, new_count):
    """Rule 2 on a stream whose budget was positive -> (table, stats)."""
    t = copy(t)
    n, before = max(int(new_count), 0), t["count"]
    new_pts = np.asarray(new_pts, F32).reshape(-1, 2)
    t["ids"][:n] = (np.arange(n, dtype=np.int64) + t["next_id"]).astype(np.uint32)
    t["age"][:n] = 0; t["birth_step"][:n] = t["step"]
    t["birth_xy"][:n] = new_pts[:n]; t["flow_xy"][:n] = 0
    t["next_id"] = (t["next_id"] + n) & 0xFFFFFFFF
    t["count"] = n
    return t, np.array([n, 0, before, n, 0, t["step"], np.uint32(t["next_id"]).astype(np.int32), 0], np.int32)


def seeded_rows(pts, n, age, flow_xy, gain):
    """Rule 5's test: (rows < n that start at their point plus gain * flow, that start [n,2] f32)."""
    p = np.asarray(pts, F32).reshape(-1, 2)[:n]
    with np.errstate(all="ignore"):
        s = (p + (F32(gain) * np.asarray(flow_xy, F32)[:n]).astype(F32)).astype(F32)
        ok = (np.abs(s[:, 0]) <= F32(1e6)) & (np.abs(s[:, 1]) <= F32(1e6))                  # False for NaN and infinity
    return (np.asarray(age)[:n] >= 1) & ok, s


def seed_points(pts, n, age, flow_xy, gain=1.0, model_seed=None):
    """Rule 5: LK's start positions [len(pts),2] f32; rows >= n, and age-0 rows, are model_seed's (None: the points)."""
    p = np.asarray(pts, F32).reshape(-1, 2)
    out = p.copy() if model_seed is None else np.asarray(model_seed, F32).reshape(-1, 2).copy()
    on, s = seeded_rows(p, n, age, flow_xy, gain)
    old = np.asarray(age)[:n] >= 1
    out[:n][old] = np.where(on[old][:, None], s[old], p[:n][old])
    return out


def update(t, prev_pts, next_pts, status, new_pts=None, new_count=None, max_total=None, seed=False, gain=1.0):
    """Rules 3 and 6 -> (table, step_ids [n_old] u32, stats [8] i32).  n_old is the table's count."""
    t = copy(t)
    n = t["count"]
    S = len(t["ids"])
    max_total = S if max_total is None else int(max_total)
    prev = np.asarray(prev_pts, F32).reshape(-1, 2)[:n]; nxt = np.asarray(next_pts, F32).reshape(-1, 2)[:n]
    keep = np.flatnonzero(np.asarray(status).ravel()[:n] != 0)
    step_ids = t["ids"][:n].copy()
    on, _ = seeded_rows(prev, n, t["age"], t["flow_xy"], gain)
    n_seeded = int(on.sum()) if seed else 0
    kept = len(keep)
    with np.errstate(all="ignore"):
        flow = (nxt[keep] - prev[keep]).astype(F32)
    for k in ("ids", "birth_step", "birth_xy"):
        t[k][:kept] = t[k][keep]
    t["age"][:kept] = t["age"][keep] + 1
    t["flow_xy"][:kept] = flow
    extra = 0 if new_count is None else max(0, min(int(new_count), max_total - kept))
    if extra:
        new_pts = np.asarray(new_pts, F32).reshape(-1, 2)
        t["ids"][kept:kept + extra] = (np.arange(extra, dtype=np.int64) + t["next_id"]).astype(np.uint32)
        t["age"][kept:kept + extra] = 0; t["birth_step"][kept:kept + extra] = t["step"] + 1
        t["birth_xy"][kept:kept + extra] = new_pts[:extra]; t["flow_xy"][kept:kept + extra] = 0
    t["next_id"] = (t["next_id"] + extra) & 0xFFFFFFFF
    t["step"] += 1
    t["count"] = kept + extra
    oldest = int(t["age"][:t["count"]].max()) if t["count"] else 0
    stats = np.array([t["count"], kept, n - kept, extra, oldest, t["step"], np.uint32(t["next_id"]).astype(np.int32), n_seeded], np.int32)
    return t, step_ids, stats


# ---------------------------------------------------------------------------------------- the ramp experiment
H_EXP, W_EXP, MARGIN = 480, 640, 420
RAMP = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.0, 1.0)
EXP_ROWS = ("yaw0.15", "pitchroll", "translation")
SEEDED_MIN_GOOD = lsr.SEEDED_MIN_GOOD       # seeded maxLevel 1: good on at least this share of the inside corners, every step, every row
PLAIN_GAP = 0.1                             # last step: plain maxLevel 3's share lies at least this far below the seeded maxLevel-1 share
EXP_LK = lsr.EXP_LK
_seqs = {}


def experiment_sequence(name):
    """The 13 gray frames of a row, the homography of each of its 12 steps and the 300 corners of frame 0 (cached per process)."""
    if name not in _seqs:
        from __graft_entry__ import load_package
        load_package()
        from of_amd import synth
        _, v, omega = next(r for r in lsr.ROWS if r[0] == name)[:3]
        T = synth.make_texture(H_EXP + 2 * MARGIN, W_EXP + 2 * MARGIN, 11)
        yy, xx = np.mgrid[0:H_EXP, 0:W_EXP].astype(np.float64)
        Hs = [synth.pixel_homography(s * np.asarray(v), s * np.asarray(omega), 1.0, (0, 0, 1), 1.0 / 640, 320, 240) for s in RAMP]
        frames, Hk = [], np.eye(3)
        for k in range(len(RAMP) + 1):
            Hi = np.linalg.inv(Hk)
            den = Hi[2, 0] * xx + Hi[2, 1] * yy + Hi[2, 2]
            sx = (Hi[0, 0] * xx + Hi[0, 1] * yy + Hi[0, 2]) / den + MARGIN
            sy = (Hi[1, 0] * xx + Hi[1, 1] * yy + Hi[1, 2]) / den + MARGIN
            frames.append(np.clip(np.rint(synth._bilinear(T, sx, sy)), 0, 255).astype(np.uint8))
            if k < len(RAMP):
                Hk = Hs[k] @ Hk
        pts = io.good_features(frames[0], 300, 0.01, 10, 7).reshape(-1, 2)
        _seqs[name] = dict(frames=frames, H=Hs, pts=pts, true_flow=synth.true_flow_px)
    return _seqs[name]


def step_points(seq, k, prev_pts):
    """lk_seed_reference.good_points' record of step k for the points it starts from."""
    flow = seq["true_flow"](seq["H"][k], prev_pts)
    end = prev_pts.astype(np.float64) + flow
    inside = (end[:, 0] >= 8) & (end[:, 0] <= W_EXP - 1 - 8) & (end[:, 1] >= 8) & (end[:, 1] <= H_EXP - 1 - 8)
    return dict(pts=prev_pts, flow=flow, inside=inside)


def cpu_lk(g0, g1, pts, max_level, seed):
    """The CPU reference tracker: plain when seed is None, else started at seed."""
    if seed is None:
        n, s, _ = lsr.lk_pyr(g0, g1, pts, max_level=max_level, **EXP_LK)
    else:
        n, s, _ = lsr.lk_pyr(g0, g1, pts, max_level=max_level, seed=seed, flags=lsr.USE_INITIAL_FLOW, **EXP_LK)
    return n.reshape(-1, 2), s.ravel()


def run_experiment(name, max_level, seeded, lk=cpu_lk):
    """One row through its 12 steps with a track table and no re-detection: every step tracks the kept points of the one before.
    seeded: from the second step on LK starts at each track's point plus its last flow (the first step is the plain maxLevel-3
    call); else every step is the plain call at max_level.  lk(g0, g1, pts [n,2], max_level, seed [n,2] or None) -> (next [n,2],
    status [n]).  -> [(good, inside)] per step."""
    seq = experiment_sequence(name)
    pts = seq["pts"].copy()
    t, _ = begin(pts, len(pts))
    out = []
    for k in range(len(RAMP)):
        n = t["count"]
        if n == 0:
            out.append((0, 0))
            continue
        first = seeded and k == 0
        seed = seed_points(pts, n, t["age"], t["flow_xy"]) if seeded and not first else None
        nxt, st = lk(seq["frames"][k], seq["frames"][k + 1], pts[:n], 3 if first else max_level, None if seed is None else seed[:n])
        out.append(lsr.good_points(step_points(seq, k, pts[:n]), nxt, st))
        t, _, _ = update(t, pts[:n], nxt, st)
        pts = nxt[st != 0]
    return out


def shares(rows):
    return [g / i if i else 1.0 for g, i in rows]
