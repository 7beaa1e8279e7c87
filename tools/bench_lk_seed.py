#!/usr/bin/env python3
"""What seeding LK from the sensor model (ofk_set_lk_seed) costs and buys on the device, at the shapes of bench.py's configs
c1 (1080p, 500 corners, 512 pairs, one slice) and c2 (640x480, 500 corners, 1024 pairs, two slices).

Variants: plain maxLevel 3 (the default path), seeded maxLevel 3, seeded 1, seeded 0 - alternated inside one process, `--rounds`
times each.  Per variant and round: the LK stage in milliseconds per step (ofk_profile_*: device events around the stage, the
seed kernel included), the whole step (wall clock around `--steps` queued steps between two syncs: the C ABI has no device event
for a whole step, and with >= 20 steps in flight the queue never runs dry), and the share of good points - status 1 and within
0.5 px of synth.true_flow_px, over the corners whose true end point lies inside the frame by 8 px - counted on the pairs that
are rendered (synth.make_batch shifts the others cyclically: they have no exact flow).
Frames: synth.make_batch; sensors: the pairs' true motion, prior velocity included.

  python tools/bench_lk_seed.py [--config c1|c2|both] [--motion default|yaw0.08|...] [--batch N] [--out profiles/lk_seed_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

SHAPES = {"c1": dict(h=1080, w=1920, corners=500, batch=512, streams=1), "c2": dict(h=480, w=640, corners=500, batch=1024, streams=2)}
MOTIONS = {
    "default": dict(v=(0.002, -0.0015, 0.001), omega=(0.002, -0.001, 0.003)),          # bench.py's
    "yaw0.08": dict(v=(0.003, -0.002, 0.001), omega=(0.002, -0.001, 0.08)),
    "pitchroll": dict(v=(0.003, -0.002, 0.001), omega=(0.06, -0.04, 0.003)),
    "translation": dict(v=(0.08, -0.05, 0.001), omega=(0.002, -0.001, 0.003)),
}
VARIANTS = (("plain L3", "off", 3), ("seeded L3", "model", 3), ("seeded L1", "model", 1), ("seeded L0", "model", 0))


def good_share(out, base, h, w):
    from of_amd import synth
    good = inside = 0
    for b, pair in enumerate(base):
        n = int(out["counts"][b])
        p = out["prev_pts"][b, :n].astype(np.float64)
        end = p + synth.true_flow_px(pair["H"], p)
        ins = (end[:, 0] >= 8) & (end[:, 0] <= w - 9) & (end[:, 1] >= 8) & (end[:, 1] <= h - 9)
        d = np.linalg.norm(out["next_pts"][b, :n].astype(np.float64) - end, axis=1)
        good += int(np.sum(ins & (out["status"][b, :n] == 1) & (d <= 0.5))); inside += int(ins.sum())
    return good, inside


def run(name, motion, batch, steps, rounds):
    import of_amd.ofk as ofk
    from of_amd import synth
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    S = SHAPES[name]
    h, w = S["h"], S["w"]
    batch = batch or S["batch"]
    prev, nxt, base = synth.make_batch(batch, h, w, seed=2000, distinct=4, d=1.0, margin=200, **MOTIONS[motion])
    p0 = base[0]
    sensors = ofk.make_sensors(batch, d=p0["d"], normal=p0["n"], omega=p0["omega"], scaling=p0["scaling"], cx=p0["cx"], cy=p0["cy"], v_prior=p0["v"])
    cfgs = {L: PipelineConfig(max_corners=S["corners"], quality=0.01, min_distance=10, block_size=7, win=15, max_level=L, max_count=20, eps=0.03)
            for L in (0, 1, 3)}
    pipe = FlowPipeline(w, h, batch, cfgs[3], streams=S["streams"])
    res = {v[0]: dict(lk_ms=[], step_ms=[]) for v in VARIANTS}
    try:
        pipe.upload(prev, nxt, sensors)
        for _ in range(rounds):
            for label, mode, L in VARIANTS:
                params = cfgs[L].to_params()
                pipe.ctx.set_lk_seed(mode, 1.0)
                for _ in range(3):
                    pipe.ctx.pairs_run(params)
                pipe.sync()
                pipe.ctx.profile_read(); pipe.ctx.profile_enable(1 << ofk.STAGES.index("lk"))
                t0 = time.perf_counter()
                for _ in range(steps):
                    pipe.ctx.pairs_run(params)
                pipe.sync()
                dt = time.perf_counter() - t0
                prof = pipe.ctx.profile_read()
                pipe.ctx.profile_enable(0)
                res[label]["lk_ms"].append(round(prof["lk"][0] / steps, 4)); res[label]["step_ms"].append(round(dt / steps * 1e3, 4))
                if "good" not in res[label]:
                    out = pipe.ctx.pairs_download()
                    g, ins = good_share(out, base, h, w)
                    res[label].update(good=g, inside=ins, good_share=round(g / max(1, ins), 4), corners_mean=float(np.mean(out["counts"])),
                                      v_err=[round(float(np.linalg.norm(out["records"][b, :3] - base[b]["v"])), 5) for b in range(len(base))])
    finally:
        pipe.ctx.set_lk_seed("off")
        pipe.close()
    for r in res.values():
        r["lk_ms_median"] = float(np.median(r["lk_ms"])); r["step_ms_median"] = float(np.median(r["step_ms"]))
    line = dict(config=name, frame=f"{w}x{h}", pairs_per_step=batch, slices=S["streams"], motion=motion, steps=steps, rounds=rounds, variants=res)
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="both", choices=["c1", "c2", "both"])
    ap.add_argument("--motion", default="default,yaw0.08", help="comma-separated: " + ", ".join(MOTIONS))
    ap.add_argument("--batch", type=int, default=0, help="pairs per step (default: the configuration's)")
    ap.add_argument("--steps", type=int, default=20, help="queued steps per measurement (>= 20)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lk_seed_bench.json"))
    args = ap.parse_args()
    load_package()
    lines = [run(c, m, args.batch, max(20, args.steps), args.rounds) for c in (("c1", "c2") if args.config == "both" else (args.config,))
             for m in args.motion.split(",")]
    with open(args.out, "w") as f:
        json.dump({"_note": "tools/bench_lk_seed.py on one MI355X: LK stage (device events) and whole step (wall clock over queued steps) per "
                            "variant, alternated in one process; good = status 1 and within 0.5 px of the true flow, over the inside corners of the rendered pairs",
                   "results": lines}, f, indent=1)


if __name__ == "__main__":
    main()
