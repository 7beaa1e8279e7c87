#!/usr/bin/env python3
"""What the exclusion zones (ofk_set_zones) cost on the device: the fused stream step of 64 streams at 1080p (500 corners,
min_features 450) and at 640x480 (200 corners, min_features 180), robust solve with drop, on the moving-object sequence of
tests/robust_stream_oracle.py (restated here; at 1080p the ground is rendered at that size for the one camera and the object is
repeated at the offset of every 480 x 640 tile that fits, six objects; the same frames in every stream).

Per step: wall clock around one synchronous step_fused, in milliseconds, and whether the step re-detected (some stream entered it with
<= min_features tracks).
  1. zones off against a checkout of the parent commit (`--parent DIR`, built), in alternating processes: both spreads.
  2. in one process, `--rounds` runs of the sequence each: off; on.  The added time of a step that does not re-detect (the update
     kernel alone) and of one that does (update, zone mask, ageing) is the difference of the medians of the two kinds of step;
     re-detections per 100 steps with and without zones.
The step's wall clock includes the frames' upload (400 MB at 1080p), so every added time stands next to the spreads of the two
medians it is the difference of.

  python tools/bench_zones.py [--parent DIR] [--config c1|c2|both] [--out profiles/zones_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"c1": dict(h=1080, w=1920, corners=500, min_features=450), "c2": dict(h=480, w=640, corners=200, min_features=180)}
MOTION = dict(v=(0.004, -0.003, 0.002), omega=(0.003, -0.002, 0.004), d=1.0)
OBJECT_SIZE, OBJECT_AT, OBJECT_STEP = (160, 220), np.array([60, 200]), np.array([5, -7])
ROBUST = dict(robust="tukey", robust_c=4.685, robust_iters=5, robust_hypotheses=64, robust_seed=0x1234ABCD5678, robust_drop=True)


def sequence(synth, h, w, seed, n_frames):
    """The scene of one camera at h x w with an object that crosses the view on its own in every 480 x 640 tile that fits."""
    frames, info = synth.render_sequence(h, w, seed, n_frames, margin=200, **MOTION)
    frames = frames.copy()
    oh, ow = OBJECT_SIZE
    tex = synth.render_pair(oh + 40, ow + 40, seed + 100, margin=96)["prev"][20:20 + oh, 20:20 + ow]
    for t in range(n_frames):
        for ty in range(0, h - 479, 480):
            for tx in range(0, w - 639, 640):
                r, c = OBJECT_AT + t * OBJECT_STEP + (ty, tx)
                frames[t, r:r + oh, c:c + ow] = tex
    return frames, info


def run_sequence(ofk, S, seq, info, streams, zones):
    """-> per step (ms, re-detected) over frames 2.. of the sequence (the first step pays the lazy allocations)."""
    from of_amd.pipeline import FlowStream, PipelineConfig, FusionConfig
    h, w = S["h"], S["w"]
    cfg = PipelineConfig(max_corners=S["corners"], quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03, **ROBUST)
    sensors = ofk.make_sensors(streams, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"])
    fs = FlowStream(w, h, batch=streams, cfg=cfg, min_features=S["min_features"], mask_radius=15, fusion=FusionConfig(use_imu=False))
    rows = []
    try:
        if zones:
            fs.ctx.set_zones(mode="hull")
        _, counts = fs.begin(np.ascontiguousarray(np.broadcast_to(seq[0], (streams, h, w, 3))))
        for t in range(1, len(seq)):
            frame = np.ascontiguousarray(np.broadcast_to(seq[t], (streams, h, w, 3)))
            few = bool((counts <= S["min_features"]).any())
            t0 = time.perf_counter()
            counts = fs.step_fused(frame, sensors)[3]
            rows.append(((time.perf_counter() - t0) * 1e3, few))
        live = int(fs.zones()["stats"][:, 0].max()) if zones else 0
    finally:
        fs.close()
    return rows[1:], live


def worker(root, name, what, frames_n, rounds, streams):
    """One process on the package under `root`: what = "off" (which a parent checkout can run too) or "both"."""
    sys.path.insert(0, root)
    from __graft_entry__ import load_package
    load_package()
    import of_amd.ofk as ofk
    from of_amd import synth
    S = SHAPES[name]
    seq, info = sequence(synth, S["h"], S["w"], 900, frames_n)
    res = {}
    for _ in range(rounds):
        for label, zones in ((("off", False),) if what == "off" else (("off", False), ("on", True))):
            rows, live = run_sequence(ofk, S, seq, info, streams, zones)
            r = res.setdefault(label, dict(plain_ms=[], redetect_ms=[], steps=0, redetections=0, live_zones=0))
            r["plain_ms"] += [round(ms, 4) for ms, few in rows if not few]; r["redetect_ms"] += [round(ms, 4) for ms, few in rows if few]
            r["steps"] += len(rows); r["redetections"] += sum(few for _, few in rows); r["live_zones"] = max(r["live_zones"], live)
    print("RESULT " + json.dumps(dict(config=name, frame=f"{S['w']}x{S['h']}", streams=streams, corners=S["corners"], min_features=S["min_features"],
                                      frames=frames_n, results=res)), flush=True)


def spawn(root, name, args, what):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", what, "--root", root, "--config", name, "--frames", str(args.frames),
           "--rounds", str(args.rounds), "--streams", str(args.streams)]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.timeout, check=True).stdout
    print(f"[{name}] {what} on {root}: done", file=sys.stderr, flush=True)
    return json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])


def spread(v):
    return dict(min=float(np.min(v)), median=float(np.median(v)), max=float(np.max(v)), n=len(v)) if len(v) else None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="both", choices=["c1", "c2", "both"])
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit: `off` is measured against it in alternating processes")
    ap.add_argument("--frames", type=int, default=24, help="frames of the sequence")
    ap.add_argument("--rounds", type=int, default=2, help="runs of the sequence per setting and process")
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--alternations", type=int, default=2, help="processes per side of the parent comparison")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per worker process")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "zones_bench.json"))
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.root, args.config, args.worker, args.frames, args.rounds, args.streams)
    lines = []
    for name in (("c1", "c2") if args.config == "both" else (args.config,)):
        line = dict(config=name)
        if args.parent:
            sides = {"parent": [], "this": []}
            for _ in range(args.alternations):
                for side, root in (("parent", os.path.abspath(args.parent)), ("this", HERE)):
                    r = spawn(root, name, args, "off")["results"]["off"]
                    sides[side] += r["plain_ms"] + r["redetect_ms"]
            p, t = spread(sides["parent"]), spread(sides["this"])
            line["off_vs_parent"] = dict(parent=p, this=t, off_inside_parent_spread=bool(p["min"] <= t["median"] <= p["max"]))
        r = spawn(HERE, name, args, "both")
        for v in r["results"].values():
            v["plain"], v["redetect"] = spread(v.pop("plain_ms")), spread(v.pop("redetect_ms"))
            v["redetections_per_100_steps"] = round(100.0 * v["redetections"] / max(1, v["steps"]), 1)
        off, on = r["results"]["off"], r["results"]["on"]
        r["added_ms"] = {k: None if off[k] is None or on[k] is None else
                         dict(median=round(on[k]["median"] - off[k]["median"], 4), off_min_max=[off[k]["min"], off[k]["max"]], on_min_max=[on[k]["min"], on[k]["max"]])
                         for k in ("plain", "redetect")}
        line.update(r)
        print(json.dumps(line), flush=True)
        lines.append(line)
        with open(args.out, "w") as f:                           # after every configuration: a later one that fails loses nothing
            json.dump({"_note": "tools/bench_zones.py on one MI355X: wall clock per synchronous fused stream step of 64 streams in ms (the frames' "
                                "upload is inside it); plain = a step that does not re-detect (zones on: the update kernel runs), redetect = one "
                                "that does (update, zone mask, ageing); added_ms = median with zones minus median without, beside both spreads; "
                                "off_vs_parent: zones off in this tree and in the parent commit in alternating processes; at 1080p the moving object is repeated in "
                                "every 480 x 640 tile (six that fit) over one camera's ground", "results": lines}, f, indent=1)


if __name__ == "__main__":
    main()
