#!/usr/bin/env python3
"""What the lighting-insensitive LK (ofk_set_lk_light) costs on the device: the frame-pair step of bench.py (ofk_pairs_run on resident
pairs, no ingest) at 512 x 1080p on one slice and at 1024 x 640 x 480 on two, 500 corners, 3-level pyramid, window 15.

A step sample is the wall clock of `--steps` queued steps that ends in a device synchronise, in milliseconds per step, behind
`--warmup` steps of the same setting; an LK-stage sample is the device time between the events around the stage (ofk_profile_*; the
stage holds the backward pass and the gate kernel of a forward-backward gate) over `--steps` steps of a pass of its own, so the
events do not sit in the step samples.  `--rounds` samples per setting and process.
  1. setting off against a checkout of the parent commit (`--parent DIR`, built), in alternating processes: both spreads; the pass
     condition is the project's usual one, the off median inside the parent's own min-max.
  2. in one process, the settings taking turns: off, bias, gain; and the same three with a plain forward-backward gate behind LK
     (fb, fb_bias, fb_gain), whose backward pass tracks under the same mode.
With the setting off the tracker is k_lk15q (four points per wave); with it on it is k_lk_light<15> (one wave per point).

  python tools/bench_lk_light.py [--parent DIR] [--config c1|c2|both] [--out profiles/lk_light_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"c1": dict(h=1080, w=1920, batch=512, streams=1), "c2": dict(h=480, w=640, batch=1024, streams=2)}
TRUTH = dict(v=(0.002, -0.0015, 0.001), omega=(0.002, -0.001, 0.003), d=1.0)
SETTINGS = (("off", None, False), ("bias", "bias", False), ("gain", "gain", False), ("fb", None, True), ("fb_bias", "bias", True),
            ("fb_gain", "gain", True))


def worker(root, name, what, steps, warmup, rounds, batch):
    """One process on the package under `root`: what = "off" (which a parent checkout can run too) or "all"."""
    sys.path.insert(0, root)
    from __graft_entry__ import load_package
    load_package()
    import of_amd.ofk as ofk
    from of_amd import synth
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    S = SHAPES[name]
    H, W, B = S["h"], S["w"], batch or S["batch"]
    cfg = PipelineConfig(max_corners=500, quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)
    prev, nxt, base = synth.make_batch(B, H, W, seed=2000, distinct=4, **TRUTH)
    if what != "off":                                            # an exposure step between the two frames: what the setting is for
        lut = synth.apply_exposure(np.arange(256, dtype=np.uint8).reshape(1, 256), 1.25, 10.0).ravel()     # no vignette: a map of pixel values
        for b in range(B):
            nxt[b] = lut[nxt[b]]
    p0 = base[0]
    sensors = ofk.make_sensors(B, d=p0["d"], normal=p0["n"], omega=p0["omega"], scaling=p0["scaling"], cx=p0["cx"], cy=p0["cy"], v_prior=p0["v"])
    pipe = FlowPipeline(W, H, B, cfg, streams=S["streams"])
    res, lk = {}, {}
    try:
        pipe.upload(prev, nxt, sensors)
        del prev, nxt

        def sync():
            pipe.ctx._ck(pipe.ctx._L.ofk_device_sync())

        for _ in range(rounds):                                  # the settings take turns, so a drift of the machine meets all of them
            for label, light, fb in (SETTINGS[:1] if what == "off" else SETTINGS):
                if what != "off":
                    pipe.ctx.set_lk_light(light)
                    pipe.ctx.set_track_gate(ofk.track_gate_setting("plain", 0.5) if fb else None)
                for _ in range(warmup):
                    pipe.run_async()
                sync()
                t0 = time.perf_counter()
                for _ in range(steps):
                    pipe.run_async()
                sync()
                res.setdefault(label, []).append(round((time.perf_counter() - t0) * 1e3 / steps, 5))
                if what != "off":                                # the LK stage between device events, in a pass of its own
                    pipe.ctx.profile_read(); pipe.ctx.profile_enable(1 << ofk.STAGES.index("lk"))
                    for _ in range(steps):
                        pipe.run_async()
                    sync()
                    lk.setdefault(label, []).append(round(pipe.ctx.profile_read()["lk"][0] / steps, 5))
                    pipe.ctx.profile_enable(0)
        corners = float(np.mean(pipe.ctx.pairs_download(points=False)["counts"]))
    finally:
        pipe.close()
    print("RESULT " + json.dumps(dict(config=name, frame=f"{W}x{H}", pairs=B, slices=S["streams"], steps=steps, warmup=warmup, corners_mean=round(corners, 1),
                                      ms_per_step=res, lk_stage_ms=lk)), flush=True)


def spawn(root, name, args, what):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", what, "--root", root, "--config", name, "--steps", str(args.steps), "--warmup",
           str(args.warmup), "--rounds", str(args.rounds), "--batch", str(args.batch)]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.timeout, check=True).stdout
    print(f"[{name}] {what} on {root}: done", file=sys.stderr, flush=True)
    return json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])


def spread(v):
    return dict(min=float(np.min(v)), median=float(np.median(v)), max=float(np.max(v)), n=len(v))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="both", choices=["c1", "c2", "both"])
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit: `off` is measured against it in alternating processes")
    ap.add_argument("--steps", type=int, default=30, help="steps per sample")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="samples per setting and process")
    ap.add_argument("--batch", type=int, default=0, help="pairs per step (default: 512 at 1080p, 1024 at 640 x 480)")
    ap.add_argument("--alternations", type=int, default=2, help="processes per side of the parent comparison")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per worker process")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "lk_light_bench.json"))
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.root, args.config, args.worker, args.steps, args.warmup, args.rounds, args.batch)
    lines = []
    for name in (("c1", "c2") if args.config == "both" else (args.config,)):
        line = dict(config=name)
        if args.parent:
            sides = {"parent": [], "this": []}
            for _ in range(args.alternations):
                for side, root in (("parent", os.path.abspath(args.parent)), ("this", HERE)):
                    sides[side] += spawn(root, name, args, "off")["ms_per_step"]["off"]
            p, t = spread(sides["parent"]), spread(sides["this"])
            line["off_vs_parent"] = dict(parent=p, this=t, off_inside_parent_spread=bool(p["min"] <= t["median"] <= p["max"]))
        r = spawn(HERE, name, args, "all")
        ms = {k: spread(v) for k, v in r.pop("ms_per_step").items()}
        lk = {k: spread(v) for k, v in r.pop("lk_stage_ms").items()}
        r["ms_per_step"], r["lk_stage_ms"] = ms, lk
        r["added_ms"] = {k: dict(step=round(ms[k]["median"] - ms[base]["median"], 5), lk_stage=round(lk[k]["median"] - lk[base]["median"], 5),
                                 lk_stage_factor=round(lk[k]["median"] / lk[base]["median"], 3))
                         for k, base in (("bias", "off"), ("gain", "off"), ("fb_bias", "fb"), ("fb_gain", "fb"))}
        line.update(r)
        print(json.dumps(line), flush=True)
        lines.append(line)
        with open(args.out, "w") as f:                           # after every configuration: a later one that fails loses nothing
            json.dump({"_note": "tools/bench_lk_light.py on one MI355X: wall clock of queued ofk_pairs_run steps up to a device synchronise, ms per step "
                                "(resident pairs, no ingest), and the LK stage between device events in a pass of its own; bias / gain = "
                                "ofk_set_lk_light, fb* = the same behind a plain forward-backward gate (the stage then holds the backward pass and "
                                "the gate kernel); added_ms = median with the setting minus median without, to be read beside the two spreads; "
                                "off_vs_parent: setting off in this tree and in the parent commit in alternating processes; the next frames of the "
                                "in-process comparison are under an exposure step of (1.25, +10)",
                       "kernels": KERNELS, "results": lines}, f, indent=1)


# registers, LDS and scratch of the new symbols (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; per FLAGS 0 / seed / eig / seed+eig)
KERNELS = {
    "k_lk_light<15>": dict(vgprs="114-121", lds_bytes=2372, scratch_bytes=0, waves_per_simd=4),
    "k_lk_light<21>": dict(vgprs="143-156", lds_bytes=3968, scratch_bytes=0, waves_per_simd=3),
    "k_lk_light<31>": dict(vgprs="222-255", lds_bytes=7556, scratch_bytes=0, waves_per_simd=2),
}


if __name__ == "__main__":
    main()
