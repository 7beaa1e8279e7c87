#!/usr/bin/env python3
"""What the epipolar solve (ofk_set_epipolar) costs on the device, at the shapes of bench.py's configs c1 (1080p, 500 corners,
512 pairs, one slice) and c2 (640x480, 500 corners, 1024 pairs, two slices).  The form of tools/bench_joint.py.

Per measurement: the whole step (wall clock around `--steps` queued steps between two syncs) and the solve stage (ofk_profile_*:
device events around the solve kernel and, with the setting on, the epipolar kernel behind it), in milliseconds per step.
  1. off against a checkout of the parent commit (`--parent DIR`, built), in alternating processes, `--rounds` each: both spreads.
  2. in one process, alternated `--rounds` times: off; epipolar with the gate open (both walks always run); epipolar with the default
     gate and a 120 px anchor; the robust solve alone; the robust solve with the epipolar solve on its weights.
  3. the fused stream step (`--streams` streams of the configuration's frame size, FusionConfig.ekf6): off against epipolar, wall
     clock per step over a short sequence.

  python tools/bench_epipolar.py [--parent DIR] [--config c1|c2|both] [--batch N] [--out profiles/epipolar_bench.json]
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
OPEN = dict(sigma_max=float("inf"))
GATED = dict(anchor=120.0)
ON_WEIGHTS = dict(sigma_max=float("inf"), weights="robust")
ROBUST = dict(loss="tukey", hypotheses=64, seed=1)


def measure(pipe, ofk, params, steps):
    for _ in range(3):
        pipe.ctx.pairs_run(params)
    pipe.sync()
    pipe.ctx.profile_read(); pipe.ctx.profile_enable(1 << ofk.STAGES.index("solve"))
    t0 = time.perf_counter()
    for _ in range(steps):
        pipe.ctx.pairs_run(params)
    pipe.sync()
    dt = time.perf_counter() - t0
    prof = pipe.ctx.profile_read()
    pipe.ctx.profile_enable(0)
    return round(dt / steps * 1e3, 4), round(prof["solve"][0] / steps, 4)


def stream_steps(ofk, S, streams, frames_n, epi):
    """Milliseconds per fused stream step over frames 1..frames_n-1 of `streams` streams (wall clock, each step synchronous)."""
    from of_amd import synth
    from of_amd.pipeline import FlowStream, PipelineConfig, FusionConfig
    h, w = S["h"], S["w"]
    seq, info = synth.render_sequence(h, w, 2100, frames_n, d=1.0, margin=200, **MOTION)
    cfg = PipelineConfig(max_corners=S["corners"], quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)
    sensors = ofk.make_sensors(streams, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"])
    fusion = FusionConfig.ekf6()
    fusion.use_imu = False; fusion.control = ofk.CONTROL_SENSORS
    fs = FlowStream(w, h, batch=streams, cfg=cfg, min_features=50, mask_radius=15, fusion=fusion)
    try:
        if epi:
            fs.ctx.set_epipolar(**epi)
        fs.begin(np.ascontiguousarray(np.broadcast_to(seq[0], (streams, h, w, 3))))
        ms = []
        for t in range(1, frames_n):
            frame = np.ascontiguousarray(np.broadcast_to(seq[t], (streams, h, w, 3)))
            t0 = time.perf_counter()
            fs.step_fused(frame, sensors)
            ms.append((time.perf_counter() - t0) * 1e3)
    finally:
        fs.close()
    return [round(v, 4) for v in ms[1:]]                         # the first step pays the lazy allocations


def worker(root, name, batch, steps, rounds, what, streams):
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
            res["off"] = dict(step_ms=[a for a, _ in m], solve_ms=[b for _, b in m])
        else:
            settings = (("off", None, None), ("epipolar, gate open", OPEN, None), ("epipolar, default gate, anchor 120 px", GATED, None),
                        ("robust", None, ROBUST), ("robust + epipolar on its weights", ON_WEIGHTS, ROBUST))
            for _ in range(rounds):
                for label, epi, rob in settings:
                    pipe.ctx.set_epipolar(None) if epi is None else pipe.ctx.set_epipolar(**epi)
                    pipe.ctx.set_robust(None) if rob is None else pipe.ctx.set_robust(**rob)
                    r = res.setdefault(label, dict(step_ms=[], solve_ms=[]))
                    a, b = measure(pipe, ofk, params, steps)
                    r["step_ms"].append(a); r["solve_ms"].append(b)
                    if epi is not None and "flags" not in r:
                        fl = pipe.structure()[0][:, 10]
                        r["flags"] = [int((fl == k).sum()) for k in (0, 1, 2, 3)]
            pipe.ctx.set_epipolar(None); pipe.ctx.set_robust(None)
    finally:
        pipe.close()
    if what == "settings" and streams > 0:
        res["fused stream step: off"] = dict(step_ms=stream_steps(ofk, S, streams, 6, None), streams=streams)
        res["fused stream step: epipolar, gate open"] = dict(step_ms=stream_steps(ofk, S, streams, 6, OPEN), streams=streams)
    print("RESULT " + json.dumps(dict(config=name, frame=f"{w}x{h}", pairs_per_step=batch, slices=S["streams"], steps=steps, results=res)), flush=True)


def spawn(root, name, args, what):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", what, "--root", root, "--config", name, "--batch", str(args.batch),
           "--steps", str(args.steps), "--rounds", str(args.rounds), "--streams", str(args.streams)]
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
    ap.add_argument("--streams", type=int, default=64, help="streams of the fused stream step measurement (0: skip it)")
    ap.add_argument("--alternations", type=int, default=3, help="processes per side of the parent comparison")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per worker process")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "epipolar_bench.json"))
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.root, args.config, args.batch, args.steps, args.rounds, args.worker, args.streams)
    lines = []
    for name in (("c1", "c2") if args.config == "both" else (args.config,)):
        line = dict(config=name)
        if args.parent:
            sides = {"parent": dict(step_ms=[], solve_ms=[]), "this": dict(step_ms=[], solve_ms=[])}
            for _ in range(args.alternations):
                for side, root in (("parent", os.path.abspath(args.parent)), ("this", HERE)):
                    r = spawn(root, name, args, "off")["results"]["off"]
                    sides[side]["step_ms"] += r["step_ms"]; sides[side]["solve_ms"] += r["solve_ms"]
            for s in sides.values():
                s["step"] = spread(s["step_ms"]); s["solve"] = spread(s["solve_ms"])
            p, t = sides["parent"], sides["this"]
            line["off_vs_parent"] = dict(sides, off_inside_parent_spread=dict(
                step=bool(p["step"]["min"] <= t["step"]["median"] <= p["step"]["max"]),
                solve=bool(p["solve"]["min"] <= t["solve"]["median"] <= p["solve"]["max"])))
        r = spawn(HERE, name, args, "settings")
        for v in r["results"].values():
            v["step"] = spread(v["step_ms"])
            if "solve_ms" in v:
                v["solve"] = spread(v["solve_ms"])
        line.update(r)
        print(json.dumps(line), flush=True)
        lines.append(line)
        with open(args.out, "w") as f:                           # after every configuration: a later one that fails loses nothing
            json.dump({"_note": "tools/bench_epipolar.py on one MI355X: whole step (wall clock over queued steps) and solve stage (device events; with the "
                                "setting on the epipolar kernel is inside it) in ms per step; off_vs_parent: the default path of this tree and of "
                                "the parent commit in alternating processes; the other settings alternated inside one process; the fused stream "
                                "step is wall clock per synchronous step; flags: pairs with epipolar flag 0, 1, 2, 3", "results": lines}, f, indent=1)


if __name__ == "__main__":
    main()
