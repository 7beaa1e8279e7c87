#!/usr/bin/env python3
"""What the corner grid (ofk_set_corner_grid) costs on the device, at the shapes of bench.py's configs c1 (1080p, 500 corners,
512 pairs, one slice) and c2 (640x480, 500 corners, 1024 pairs, two slices).

Per measurement: the whole step (wall clock around `--steps` queued steps between two syncs) and the selection stage
(ofk_profile_*: device events around the three selection kernels), in milliseconds per step.
  1. off against a checkout of the parent commit (`--parent DIR`, built), in alternating processes, `--rounds` each: both spreads.
  2. in one process, alternated `--rounds` times: off; a grid that binds on bench.py's texture (cell 64, cap ~ 2 maxCorners / cells);
     and, on the concentrated-contrast scene (band-limited noise at amplitude 12 with one box of amplitude 55 over 15 % of the frame,
     the 640x480 scene tiled to size), plain, the grid, and the grid with max_rank = 8 maxCorners - the deep walk.
     With each grid setting: the statistics (accepted, examined) over the batch.

  python tools/bench_corner_grid.py [--parent DIR] [--config c1|c2|both] [--batch N] [--out profiles/corner_grid_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"c1": dict(h=1080, w=1920, corners=500, batch=512, streams=1), "c2": dict(h=480, w=640, corners=500, batch=1024, streams=2)}
MOTION = dict(v=(0.002, -0.0015, 0.001), omega=(0.002, -0.001, 0.003))               # bench.py's
CELL = 64


def concentrated(h, w, batch):
    """The 640x480 scene tiled to h x w, as BGR pairs: the next frame is the previous one moved by (2, 1) pixels."""
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import corner_grid_cases as K                                # the one definition of the scene (tests/corner_grid_cases.py: QUALITY_SCENE)
    tile = K.scene("quality")
    g = np.tile(tile, (-(-h // 480), -(-w // 640)))[:h, :w]
    prev = np.repeat(g[:, :, None], 3, 2); nxt = np.roll(g, (1, 2), (0, 1)); nxt = np.repeat(nxt[:, :, None], 3, 2)
    return np.broadcast_to(prev, (batch, h, w, 3)), np.broadcast_to(nxt, (batch, h, w, 3))


def measure(pipe, ofk, params, steps):
    for _ in range(3):
        pipe.ctx.pairs_run(params)
    pipe.sync()
    pipe.ctx.profile_read(); pipe.ctx.profile_enable(1 << ofk.STAGES.index("select"))
    t0 = time.perf_counter()
    for _ in range(steps):
        pipe.ctx.pairs_run(params)
    pipe.sync()
    dt = time.perf_counter() - t0
    prof = pipe.ctx.profile_read()
    pipe.ctx.profile_enable(0)
    return round(dt / steps * 1e3, 4), round(prof["select"][0] / steps, 4)


def worker(root, name, batch, steps, rounds, what):
    """One process on the package under `root`: what = "off" (the default path alone, which a parent checkout has too) or "settings"."""
    sys.path.insert(0, root)
    from __graft_entry__ import load_package
    load_package()
    import of_amd.ofk as ofk
    from of_amd import synth
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    S = SHAPES[name]
    h, w, batch = S["h"], S["w"], batch or S["batch"]
    cfg = PipelineConfig(max_corners=S["corners"], quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)
    params = cfg.to_params()
    prev, nxt, base = synth.make_batch(batch, h, w, seed=2000, distinct=4, d=1.0, margin=200, **MOTION)
    p0 = base[0]
    sensors = ofk.make_sensors(batch, d=p0["d"], normal=p0["n"], omega=p0["omega"], scaling=p0["scaling"], cx=p0["cx"], cy=p0["cy"])
    pipe = FlowPipeline(w, h, batch, cfg, streams=S["streams"])
    res = {}
    try:
        pipe.upload(prev, nxt, sensors)
        if what == "off":
            m = [measure(pipe, ofk, params, steps) for _ in range(rounds)]
            res["off"] = dict(step_ms=[a for a, _ in m], select_ms=[b for _, b in m])
        else:
            cells = -(-w // CELL) * -(-h // CELL)
            cap = max(1, round(2 * S["corners"] / cells))
            scenes = (("bench texture", None, (("off", None), ("grid", dict(cell=CELL, cap=cap)))),
                      ("concentrated", concentrated(h, w, batch), (("off", None), ("grid", dict(cell=CELL, cap=cap)),
                                                                   ("grid max_rank", dict(cell=CELL, cap=cap, max_rank=8 * S["corners"])))))
            for scene, frames, settings in scenes:
                if frames is not None:
                    pipe.upload(np.ascontiguousarray(frames[0]), np.ascontiguousarray(frames[1]), sensors)
                for _ in range(rounds):
                    for label, kw in settings:
                        pipe.ctx.set_corner_grid(None) if kw is None else pipe.ctx.set_corner_grid(**kw)
                        r = res.setdefault(f"{scene}: {label}", dict(step_ms=[], select_ms=[], setting=kw))
                        a, b = measure(pipe, ofk, params, steps)
                        r["step_ms"].append(a); r["select_ms"].append(b)
                        if "corners_mean" not in r:
                            out = pipe.ctx.pairs_download(points=False)
                            r["corners_mean"] = round(float(out["counts"].mean()), 2)
                            if kw is not None:
                                st = pipe.corner_grid_stats()
                                r.update(examined_mean=round(float(st[:, 1].mean()), 1), examined_max=int(st[:, 1].max()))
                pipe.ctx.set_corner_grid(None)
    finally:
        pipe.close()
    print("RESULT " + json.dumps(dict(config=name, frame=f"{w}x{h}", pairs_per_step=batch, slices=S["streams"], steps=steps, results=res)), flush=True)


def spawn(root, name, args, what):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", what, "--root", root, "--config", name, "--batch", str(args.batch),
           "--steps", str(args.steps), "--rounds", str(args.rounds)]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.timeout, check=True).stdout
    print(f"[{name}] {what} on {root}: done", file=sys.stderr, flush=True)
    return json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])


def spread(v):
    return dict(min=float(np.min(v)), median=float(np.median(v)), max=float(np.max(v)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="both", choices=["c1", "c2", "both"])
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit: `off` is measured against it in alternating processes")
    ap.add_argument("--batch", type=int, default=0, help="pairs per step (default: the configuration's)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--alternations", type=int, default=3, help="processes per side of the parent comparison")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per worker process")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "corner_grid_bench.json"))
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.root, args.config, args.batch, args.steps, args.rounds, args.worker)
    lines = []
    for name in (("c1", "c2") if args.config == "both" else (args.config,)):
        line = dict(config=name)
        if args.parent:
            sides = {"parent": dict(step_ms=[], select_ms=[]), "this": dict(step_ms=[], select_ms=[])}
            for _ in range(args.alternations):
                for side, root in (("parent", os.path.abspath(args.parent)), ("this", HERE)):
                    r = spawn(root, name, args, "off")["results"]["off"]
                    sides[side]["step_ms"] += r["step_ms"]; sides[side]["select_ms"] += r["select_ms"]
            for s in sides.values():
                s["step"] = spread(s["step_ms"]); s["select"] = spread(s["select_ms"])
            p, t = sides["parent"], sides["this"]
            line["off_vs_parent"] = dict(sides, off_inside_parent_spread=dict(
                step=bool(p["step"]["min"] <= t["step"]["median"] <= p["step"]["max"]),
                select=bool(p["select"]["min"] <= t["select"]["median"] <= p["select"]["max"])))
        r = spawn(HERE, name, args, "settings")
        for v in r["results"].values():
            v["step"] = spread(v["step_ms"]); v["select"] = spread(v["select_ms"])
        line.update(r)
        print(json.dumps(line), flush=True)
        lines.append(line)
        with open(args.out, "w") as f:                           # after every configuration: a later one that fails loses nothing
            json.dump({"_note": "tools/bench_corner_grid.py on one MI355X: whole step (wall clock over queued steps) and selection stage (device "
                                "events) in ms per step; off_vs_parent: the default path of this tree and of the parent commit in alternating "
                                "processes; the other settings alternated inside one process", "results": lines}, f, indent=1)


if __name__ == "__main__":
    main()
