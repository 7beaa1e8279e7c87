#!/usr/bin/env python3
"""The ordered kernel launches of a tiny stream run with every per-track setting on: what a change of the host path behind the track
table, the depths, the templates, the keyframe and its rotation must leave as it was.

The run: 2 streams of 64 x 48, 16 points, the five settings on; ofk_stream_begin, then three ofk_stream_step_fused with
redetect_replace on and min_features = max_corners, so that every step's replace branch runs.

  python tools/track_state_launches.py --out FILE     runs itself under `rocprofv3 --kernel-trace` (a child process, no counters)
                                                      and writes the kernel names in launch order, one per line, to FILE
  python tools/track_state_launches.py --compare A B  the two lists are the same: prints their length, or the first difference

Take A on a built checkout of the parent commit and B on this tree; profiles/LOG.md records the outcome."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, B, PTS = 48, 64, 2, 16


def run():
    import numpy as np
    sys.path.insert(0, HERE)
    from __graft_entry__ import load_package
    load_package()
    import of_amd.ofk as ofk
    from of_amd.pipeline import FusionConfig
    rng = np.random.default_rng(17)
    big = np.kron(rng.integers(0, 256, (B, H // 4 + 1, W // 4 + 3)).astype(np.uint8), np.ones((4, 4), np.uint8))
    frames = [np.repeat(big[:, 1:H + 1, 4 - t:4 - t + W, None], 3, -1).copy() for t in range(4)]
    sensors = ofk.make_sensors(B, d=1.0, omega=(0.004, -0.003, 0.004), scaling=1.0 / 60.0, cx=W / 2.0, cy=H / 2.0)
    params = ofk.Params(PTS, 0.01, 3.0, 3, 9, 1, 20, 0.03, 1e-4, ofk.SOLVE_NODE, 0, 0.0)
    fusion = FusionConfig(use_imu=False, redetect_replace=True).to_struct()
    ctx = ofk.Context(0, W, H, B, PTS, 1)
    try:
        ctx.imu_reset(B)
        ctx.set_track_table(ofk.track_table_setting("flow"))
        ctx.set_track_depth(ofk.track_depth_setting(min_rows=3))
        ctx.set_track_template(ofk.track_template_setting(win=5, fit_min=3))
        ctx.set_keyframe(ofk.keyframe_setting(min_rows=3))
        ctx.set_keyframe_rotation(ofk.keyframe_rotation_setting(sigma_bias=1e-3))
        _, counts = ctx.stream_begin(frames[0], params)
        for t in (1, 2, 3):
            _, _, _, counts = ctx.stream_step_fused(frames[t], sensors, params, fusion, PTS, 3)
        print("counts behind the last step:", counts.tolist(), file=sys.stderr)
    finally:
        ctx.close()


def trace(out):
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
                        "--run"], check=True, timeout=300)
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if len(files) != 1:
            raise SystemExit(f"expected one kernel trace, found {files}")
        with open(files[0], newline="") as f:
            rows = sorted(csv.DictReader(f), key=lambda r: (int(r["Start_Timestamp"]), int(r["Dispatch_Id"])))
    names = [r["Kernel_Name"] for r in rows]
    with open(out, "w") as f:
        f.write("\n".join(names) + "\n")
    print(f"{len(names)} launches, {len(set(names))} kernels -> {out}")


def compare(a, b):
    la, lb = (open(p).read().split("\n") for p in (a, b))
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            raise SystemExit(f"launch {i} differs: {x} / {y}")
    if len(la) != len(lb):
        raise SystemExit(f"{len(la) - 1} launches against {len(lb) - 1}")
    print(f"identical: {len(la) - 1} launches in the same order")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--run", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.run:
        run()
    elif args.compare:
        compare(*args.compare)
    elif args.out:
        trace(args.out)
    else:
        ap.error("one of --out, --compare")
