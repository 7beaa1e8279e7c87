#!/usr/bin/env python3
"""What the rectified view (ofk_set_rectify beside ofk_set_camera and ofk_set_stabilise) and the warp through a lens (ofk_warp_lens) cost on
the device, measured as tools/bench_stabilise.py measures the plain view: the fused stream step of 64 streams at 1080p (500 corners) and at
640x480 (200 corners) on a rendered sequence (the same frames in every stream).

  1. every setting off against a checkout of the parent commit (`--parent DIR`, built), in alternating processes: both spreads.  "Off
     costs nothing" is claimed only if this tree's median lies inside the parent's own spread.
  2. in one process, `--rounds` runs of the sequence each, wall clock around one synchronous step_fused in ms: off; the track table and
     the keyframe; the same with the plain view (no camera: k_warp_u8); camera + table + keyframe; the same with the view and rectify
     (k_warp_lens_u8).  The frames are the lens-free ones in every mode (the step's work does not depend on what they show).
  3. the stage entries on 64 frames of the first configuration: ofk_warp_perspective against ofk_warp_lens (Brown, Brown with rational
     terms, fisheye) on the same matrix; the uploads and downloads are inside both, the difference of the medians is the kernels'.
The figures are recorded, not thresholded.

  python tools/bench_rectify.py [--parent DIR] [--config c1|c2|both] [--out profiles/rectify_bench.json]
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
# label -> (the track table and the keyframe, the camera, the view, rectify)
MODES = {"off": (False, False, False, False), "key": (True, False, False, False), "stab": (True, False, True, False),
         "cam_key": (True, True, False, False), "rect": (True, True, True, True)}
LENSES = {"brown": ("brown", (-0.28, 0.09, 0.0008, -0.0005, -0.012)), "brown_rational": ("brown", (-0.28, 0.09, 0.0008, -0.0005, -0.012, 0.05, -0.01, 0.002)),
          "fisheye": ("fisheye", (-0.03, 0.005, -0.001, 0.0002))}


def camera_of(info, lens="brown"):
    from of_amd.pipeline import CameraModel
    model, k = LENSES[lens]
    return CameraModel(fx=1.0 / info["scaling"], cx=info["cx"], cy=info["cy"], k=k, model=model)


def run_sequence(ofk, S, seq, info, streams, key, cam, stab, rect):
    """-> per step ms over frames 2.. of the sequence (the first step pays the lazy allocations)."""
    from of_amd.pipeline import FlowStream, PipelineConfig, FusionConfig
    h, w = S["h"], S["w"]
    cfg = PipelineConfig(max_corners=S["corners"], quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)
    sensors = ofk.make_sensors(streams, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"])
    fs = FlowStream(w, h, batch=streams, cfg=cfg, min_features=S["min_features"], mask_radius=15, fusion=FusionConfig(use_imu=False))
    rows, last = [], None
    try:
        if key:
            fs.ctx.set_track_table(seed="off")
            fs.ctx.set_keyframe(ofk.keyframe_setting())
        if cam:
            cm = camera_of(info)
            fs.ctx.set_camera(cm.setting())
        if rect:
            fs.ctx.set_rectify(ofk.rectify_setting(r_max=1.05 * cm.ideal_radius(h, w)))
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
            last = dict(flag=int(d["rec"][0][30]), rebases=int(d["rec"][0][33]), cover=int(d["covered"][0]) / float(h * w))
    finally:
        fs.close()
    return rows[1:], last


def stage_entries(ofk, S, seq, info, streams, rounds):
    """-> label -> ms per call of the stage entry over `streams` gray frames, one matrix (a small rigid motion) for all."""
    h, w = S["h"], S["w"]
    ctx = ofk.Context(0, w, h, streams, 16, 1)
    res = {}
    try:
        gray = np.ascontiguousarray(np.broadcast_to(seq[0][:, :, 1], (streams, h, w)))
        a = 0.01
        M = np.tile(np.array([[np.cos(a), -np.sin(a), 6.0], [np.sin(a), np.cos(a), -4.0], [1e-6, -1e-6, 1.0]]), (streams, 1, 1))
        calls = {"warp_perspective": lambda: ctx.warp_perspective(gray, M)}
        for lens in LENSES:
            cam = camera_of(info, lens).setting()
            calls["warp_lens_" + lens] = lambda cam=cam: ctx.warp_lens(gray, cam, M)
        for label, call in calls.items():
            call()
            for _ in range(max(3, 3 * rounds)):
                t0 = time.perf_counter()
                call()
                res.setdefault(label, []).append(round((time.perf_counter() - t0) * 1e3, 4))
    finally:
        ctx.close()
    return res


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
            rows, last = run_sequence(ofk, S, seq, info, streams, *MODES[label])
            r = res.setdefault(label, dict(ms=[]))
            r["ms"] += [round(ms, 4) for ms in rows]
            if last is not None:
                r["last_view"] = last
    out = dict(config=name, frame=f"{S['w']}x{S['h']}", streams=streams, corners=S["corners"], frames=frames_n, results=res)
    if what == "all":
        out["stage_entries_ms"] = stage_entries(ofk, S, seq, info, streams, rounds)
    print("RESULT " + json.dumps(out), flush=True)


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
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "rectify_bench.json"))
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
        r["added_ms"] = {f"{k}_minus_{base}": dict(median=round(res[k]["step"]["median"] - res[base]["step"]["median"], 4),
                                 base_min_max=[res[base]["step"]["min"], res[base]["step"]["max"]], on_min_max=[res[k]["step"]["min"], res[k]["step"]["max"]])
                         for base, k in (("key", "stab"), ("cam_key", "rect"), ("stab", "rect"))}
        r["stage_entries_ms"] = {k: spread(v) for k, v in r["stage_entries_ms"].items()}
        line.update(r)
        print(json.dumps(line), flush=True)
        lines.append(line)
        with open(args.out, "w") as f:                           # after every configuration: a later one that fails loses nothing
            json.dump({"_note": "tools/bench_rectify.py on one MI355X: wall clock per synchronous fused stream step of 64 streams in ms (the frames' upload "
                                "is inside it, the stabilised frames stay on the device); key = the track table and the keyframe, stab = the same with the "
                                "plain stabilised view, cam_key = key beside a Brown camera, rect = cam_key with the view and rectify (k_warp_lens_u8); "
                                "added_ms = median of the second minus median of the first, beside both spreads; stage_entries_ms: one call of the stage "
                                "entry over 64 gray frames, uploads and downloads inside; off_vs_parent: every setting off in this tree and in the parent "
                                "commit in alternating processes", "results": lines}, f, indent=1)


if __name__ == "__main__":
    main()
