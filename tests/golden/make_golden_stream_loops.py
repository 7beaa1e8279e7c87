#!/usr/bin/env python3
"""Pinned outputs of the video-stream checker (tests/stream_oracle.py::NodeLoop and its drivers) for tests/test_stream_loops_golden.py.

    python tests/golden/make_golden_stream_loops.py        # rewrites tests/golden/stream_loops.npz

The committed stream_loops.npz was NOT written by this file as it stands: it was recorded at commit 030326a, from the four
hand-kept loops that NodeLoop replaced (oracle_stream, oracle_node_fused, seed_stream_oracle.StreamLoop,
robust_stream_oracle.RobustLoop), by this file's form for their API; this form regenerates the same bytes in every array.  So the
fixture pins what the stream steps were checked against before the loops became one.  Outputs only, no frames.
To record it again from those loops, check out 030326a and change this file in four places:
  * define imu_messages (tests/stream_oracle.py of this commit) in this file and import seed_stream_oracle as sso;
  * seeded():  loop = sso.StreamLoop(frames[0], cfg, 59, 12)   and   v, tr, n_old, n_tr = loop.step(frames[t], s, lk), recorded as
    dict(v=v, tracks=tr, n_old=n_old, n_tracked=n_tr);
  * robust():  loop = rso.RobustLoop(frames[0], cfg, 199, 15, kind, problem, drop, model=<the ekf6 model or None>)   and
    steps.append(loop.step(frames[t], sr, msgs)) with msgs = None outside ekf6;
  * plain() and node() stay: oracle_stream and oracle_node_fused kept their signatures.

Cases (the smallest that reach every branch): plain 240x320 with re-detection on every step and on none; the same with the seeded
tracker built anew every step; the IMU state in the loop without filter, with ekf6 and with ekf6 + gps, re-detection firing;
the robust solve as step / fused / ekf6 with drop off and on, 480x640 (the object does not fit a smaller frame), seed 900, where
every kind meets tracked points of weight 0; min_features 199 of 200 corners so that re-detection fires with and without drop;
problem 1 in the fused cases, so that the hypothesis counter is covered.
Layout per case: `first`, and per field the steps' arrays concatenated flat with `<field>.size` = their sizes, -1 for None."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]
OUT = os.path.join(HERE, "stream_loops.npz")

from __graft_entry__ import load_package  # noqa: E402

load_package()
from of_amd import synth  # noqa: E402
from of_amd.pipeline import PipelineConfig, FusionConfig  # noqa: E402
import lk_seed_reference as R  # noqa: E402
import robust_stream_oracle as rso  # noqa: E402
from stream_oracle import NodeLoop, imu_messages, oracle_stream, oracle_node_fused  # noqa: E402

FIELDS = ("v", "v_uav", "x", "P", "vel", "tracks", "n_old", "n_tracked", "weights", "stats")


def pack(first, steps):
    out = {"first": first}
    for f in FIELDS:
        vals = [s.get(f) for s in steps]
        out[f + ".size"] = np.array([-1 if v is None else np.size(v) for v in vals])
        some = [np.ravel(v) for v in vals if v is not None]
        if some:
            out[f] = np.concatenate(some)
    assert out["tracks"].dtype == np.float32 and first.dtype == np.float32
    return out


def plain_inputs():
    cfg = PipelineConfig(max_corners=60, quality=0.04, min_distance=9, block_size=7, win=15, max_level=2, max_count=20, eps=0.03)
    frames, info = synth.render_sequence(240, 320, 77, 5, v=(0.03, 0.012, 0.0), omega=(0.0, 0.0, 0.01), d=1.0)
    return cfg, frames, info


def plain():
    cfg, frames, info = plain_inputs()
    s = R.experiment_sensors(info, v_prior=(0, 0, 0))
    for min_feat in (59, 10):
        first, steps = oracle_stream(frames, cfg, s, min_feat, 12)
        yield f"plain-{min_feat}", pack(first, [dict(v=v, tracks=tr, n_old=n_old, n_tracked=n_tr) for v, tr, n_old, n_tr in steps])


def seeded():
    cfg, frames, info = plain_inputs()
    s = R.experiment_sensors(info)
    loop = NodeLoop(frames[0], cfg, 59, 12)
    first = loop.tracks.copy()
    steps = []
    for t in range(1, len(frames)):
        seed = R.predict(loop.tracks, s)
        lk = lambda g0, g1, old: R.lk_pyr(g0, g1, old, cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr, seed=seed, flags=R.USE_INITIAL_FLOW)
        o = loop.step(frames[t], s, lk=lk)
        steps.append({f: o[f] for f in ("v", "tracks", "n_old", "n_tracked")})
    yield "seeded", pack(first, steps)


def node():
    nf = 6
    cfg = PipelineConfig(max_corners=120, quality=0.02, min_distance=10, block_size=7)
    frames, info = synth.render_sequence(240, 320, 940, nf, v=(0.004, -0.003, 0.002), omega=(0.002, 0.001, -0.003), d=1.0)
    statics = dict(d=1.0, offset=(0.0, 0.0, 0.1), scaling=info["scaling"], cx=info["cx"], cy=info["cy"])
    rng = np.random.default_rng(5)
    msgs = np.stack([imu_messages(rng, 100.0 + 0.1 * t, 3) for t in range(nf - 1)])
    gps = rng.normal(0.0, 0.01, (nf - 1, 3)) + [0.004, -0.003, 0.002]
    for name, model, g in (("node", None, None), ("ekf6", FusionConfig.ekf6(dt=0.1).model, None),
                           ("ekf6-gps", FusionConfig.ekf6(dt=0.1, gps=True, r=4.0, r_gps=0.5).model, gps)):
        first, steps = oracle_node_fused(frames, cfg, statics, msgs, 119, 15, model, gps=g)
        key = "vel" if model is None else "x"
        yield name, pack(first, [{"v": v, "v_uav": vu, key: vel, "tracks": tr, "n_old": n_old, "n_tracked": n_tr} for v, vu, vel, tr, n_old, n_tr in steps])


ROBUST_SEED = 900


def robust():
    from of_amd import ofk
    nf = 6
    cfg = PipelineConfig(max_corners=200, quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)
    frames, info = rso.sequence(synth, 480, 640, ROBUST_SEED, nf)
    sr = ofk.make_sensors(1, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"])[0]
    for kind, problem in (("step", 0), ("fused", 1), ("ekf6", 0)):
        for drop in (False, True):
            rng = np.random.default_rng(8)
            imu = dict(imu_offset=(0.0, 0.0, 0.1), model=FusionConfig.ekf6(dt=0.1).model) if kind == "ekf6" else {}
            loop = NodeLoop(frames[0], cfg, 199, 15, solve=rso.robust_solver(problem, drop, kind != "step"), **imu)
            first = loop.tracks.copy()
            steps = []
            for t in range(1, nf):
                msgs = imu_messages(rng, 50.0 + 0.1 * t, 3, rate=rso.MOTION["omega"], rate_sigma=0.0005) if kind == "ekf6" else ()
                o = loop.step(frames[t], sr, msgs)
                steps.append({f: o[f] for f in FIELDS if f != "vel"})
            yield f"robust-{kind}-{'drop' if drop else 'keep'}", pack(first, steps)


GROUPS = dict(plain=plain, seeded=seeded, node=node, robust=robust)


def record(group):
    return {f"{case}/{k}": a for case, arrays in GROUPS[group]() for k, a in arrays.items()}


def main():
    out = {}
    for group in GROUPS:
        out.update(record(group))
    np.savez_compressed(OUT, **out)
    for case in sorted({k.split("/")[0] for k in out}):
        n_tr, sizes = out[f"{case}/n_tracked"], out[f"{case}/tracks.size"] // 2
        zero = ""
        if f"{case}/weights" in out:
            w = np.split(out[f"{case}/weights"], np.cumsum(out[f"{case}/weights.size"])[:-1])
            zero = f", zero-weight tracked points {[int(np.count_nonzero(wi == 0)) - int(a - b) for wi, a, b in zip(w, out[f'{case}/n_old'], n_tr)]}"
        print(f"{case}: n_old {out[f'{case}/n_old'].tolist()} tracked {n_tr.tolist()} tracks {sizes.tolist()} solved {(out[f'{case}/v.size'] > 0).tolist()}{zero}")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
