#!/usr/bin/env python3
"""What a stream's stabilised view (ofk_set_stabilise) costs on the device: the fused stream step of 64 streams at 1080p (500 corners) and
at 640x480 (200 corners), as tools/bench_keyframe.py measures it, on a rendered sequence (the same frames in every stream).

Per step: wall clock around one synchronous step_fused, in milliseconds (the frames' upload is inside it; the stabilised frames stay on
the device: their download is not).
  1. every setting off against a checkout of the parent commit (`--parent DIR`, built), in alternating processes: both spreads.  "Off
     costs nothing" is claimed only if this tree's median lies inside the parent's own spread.
  2. in one process, `--rounds` runs of the sequence each: off; the track table and the keyframe (which the view needs); the same with
     the view (two more launches per step: k_stab_pose and k_warp_u8 over every stream's frame); the same two beside the keyframe
     rotation.  The added time per step is the difference of the medians, beside the spreads of the two runs it is taken from: it is
     recorded, not thresholded.

  python tools/bench_stabilise.py [--parent DIR] [--config c1|c2|both] [--out profiles/stabilise_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"c1": dict(h=1080, w=1920, corners=500, min_features=100), "c2": dict(h=480, w=640, corners=200, min_features=40)}
MOTION = dict(v=(0.004, -0.003, 0.002), omega=(0.003, -0.002, 0.004), d=1.0)
# label -> (the track table and the keyframe, the keyframe rotation, the view)
MODES = {"off": (False, False, False), "key": (True, False, False), "stab": (True, False, True), "key_rot": (True, True, False), "stab_rot": (True, True, True)}


def run_sequence(ofk, S, seq, info, streams, key, rot, stab):
    """-> (per step ms over frames 2.. of the sequence (the first step pays the lazy allocations), the last view record and cover or None)."""
    from of_amd.pipeline import FlowStream, PipelineConfig, FusionConfig
    h, w = S["h"], S["w"]
    cfg = PipelineConfig(max_corners=S["corners"], quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)
    sensors = ofk.make_sensors(streams, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"])
    fs = FlowStream(w, h, batch=streams, cfg=cfg, min_features=S["min_features"], mask_radius=15, fusion=FusionConfig(use_imu=False))
    rows, rec = [], None
    try:
        if key:
            fs.ctx.set_track_table(seed="off")
            fs.ctx.set_keyframe(ofk.keyframe_setting())
        if rot:
            fs.ctx.set_keyframe_rotation(ofk.keyframe_rotation_setting())
        if stab:
            fs.ctx.set_stabilise(ofk.stabilise_setting())
        fs.begin(np.ascontiguousarray(np.broadcast_to(seq[0], (streams, h, w, 3))))
        for t in range(1, len(seq)):
            frame = np.ascontiguousarray(np.broadcast_to(seq[t], (streams, h, w, 3)))
            t0 = time.perf_counter()
            fs.step_fused(frame, sensors)
            rows.append((time.perf_counter() - t0) * 1e3)
        if stab:
            d = fs.ctx.stab_download(streams, frames=False)
            rec = (d["rec"][0], int(d["covered"][0]))
    finally:
        fs.close()
    return rows[1:], rec


def worker(root, name, what, frames_n, rounds, streams):
    """One process on the package under `root`: what = "off" (which a parent checkout can run too) or "all"."""
    sys.path.insert(0, root)
    from __graft_entry__ import load_package
    load_package()
    import of_amd.ofk as ofk
    from of_amd import synth
    S = SHAPES[name]
    labels = ("off",) if what == "off" else tuple(MODES)
    seq, info = synth.render_sequence(S["h"], S["w"], 900, frames_n, margin=200, **MOTION)
    res = {}
    for _ in range(rounds):
        for label in labels:
            rows, rec = run_sequence(ofk, S, seq, info, streams, *MODES[label])
            r = res.setdefault(label, dict(ms=[]))
            r["ms"] += [round(ms, 4) for ms in rows]
            if rec is not None:                                  # the last step of stream 0: the view's record
                r["last_record"] = dict(M=[float(t) for t in rec[0][0:9]], flag=int(rec[0][30]), rebases=int(rec[0][33]), approx=int(rec[0][34]),
                                        cover=rec[1] / float(S["h"] * S["w"]))
    print("RESULT " + json.dumps(dict(config=name, frame=f"{S['w']}x{S['h']}", streams=streams, corners=S["corners"], frames=frames_n, results=res)), flush=True)


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
    ap.add_argument("--frames", type=int, default=16, help="frames of the sequence")
    ap.add_argument("--rounds", type=int, default=2, help="runs of the sequence per setting and process")
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--alternations", type=int, default=2, help="processes per side of the parent comparison")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per worker process")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "stabilise_bench.json"))
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
                    sides[side] += spawn(root, name, args, "off")["results"]["off"]["ms"]
            p, t = spread(sides["parent"]), spread(sides["this"])
            line["off_vs_parent"] = dict(parent=p, this=t, off_inside_parent_spread=bool(p["min"] <= t["median"] <= p["max"]))
        r = spawn(HERE, name, args, "all")
        for v in r["results"].values():
            v["step"] = spread(v.pop("ms"))
        res = r["results"]
        r["added_ms"] = {k: dict(median=round(res[k]["step"]["median"] - res[base]["step"]["median"], 4),
                                 base_min_max=[res[base]["step"]["min"], res[base]["step"]["max"]], on_min_max=[res[k]["step"]["min"], res[k]["step"]["max"]])
                         for base, k in (("off", "key"), ("key", "stab"), ("key_rot", "stab_rot"))}
        line.update(r)
        print(json.dumps(line), flush=True)
        lines.append(line)
        with open(args.out, "w") as f:                           # after every configuration: a later one that fails loses nothing
            json.dump({"_note": "tools/bench_stabilise.py on one MI355X: wall clock per synchronous fused stream step of 64 streams in ms (the frames' "
                                "upload is inside it, the stabilised frames stay on the device); key = the track table and the keyframe, stab = the same with "
                                "the stabilised view, *_rot = beside the keyframe rotation; added_ms = median of the second minus median of the first, beside "
                                "both spreads; last_record = stream 0's view record behind the last step; off_vs_parent: every setting off in this tree and "
                                "in the parent commit in alternating processes", "results": lines}, f, indent=1)


if __name__ == "__main__":
    main()
