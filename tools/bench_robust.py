#!/usr/bin/env python3
"""What the robust velocity solve (ofk_set_robust) costs on the device, at the shapes of bench.py's configs c1 (1080p, 500 corners,
512 pairs, one slice) and c2 (640x480, 500 corners, 1024 pairs, two slices).

Variants: setting off (the plain kernels), and TUKEY with K in {0, 16, 64, 256} hypotheses x {0, 5} rounds - alternated inside one
process, `--rounds` times each.  Per variant and round: the solve stage in milliseconds per step (ofk_profile_*: device events around
the stage) and the whole step (wall clock around `--steps` queued steps between two syncs).  The spread of the "off" rows over the
rounds is the run-to-run spread the other rows are read against; the same script on the parent commit (where only "off" exists: pass
--off-only) gives the figure "off" has to equal.  Every other pair carries a moving object (tests/robust_reference.py's scene), so the
reweighting has outliers to work on.

  python tools/bench_robust.py [--config c1|c2|both] [--batch N] [--off-only] [--out profiles/robust_bench.json]
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
MOTION = dict(v=(0.002, -0.0015, 0.001), omega=(0.002, -0.001, 0.003))                # bench.py's
VARIANTS = [("off", None)] + [(f"K{K} it{it}", dict(loss="tukey", hypotheses=K, iters=it, seed=1)) for K in (0, 16, 64, 256) for it in (0, 5)]


def run(name, batch, steps, rounds, off_only):
    import of_amd.ofk as ofk
    from of_amd import synth
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    S = SHAPES[name]
    h, w = S["h"], S["w"]
    batch = batch or S["batch"]
    prev, nxt, base = synth.make_batch(batch, h, w, seed=2000, distinct=4, d=1.0, margin=200, **MOTION)
    prev, nxt = prev.copy(), nxt.copy()
    tex = synth.render_pair(300, 400, 77, margin=96)["prev"][20:280, 20:350]
    for b in range(1, batch, 2):
        prev[b, 60:320, 80:410] = tex; nxt[b, 65:325, 73:403] = tex
    p0 = base[0]
    sensors = ofk.make_sensors(batch, d=p0["d"], normal=p0["n"], omega=p0["omega"], scaling=p0["scaling"], cx=p0["cx"], cy=p0["cy"], v_prior=p0["v"])
    cfg = PipelineConfig(max_corners=S["corners"], quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)
    variants = VARIANTS[:1] if off_only else VARIANTS
    pipe = FlowPipeline(w, h, batch, cfg, streams=S["streams"])
    res = {v[0]: dict(solve_ms=[], step_ms=[]) for v in variants}
    params = cfg.to_params()
    try:
        pipe.upload(prev, nxt, sensors)
        for _ in range(rounds):
            for label, setting in variants:
                if not off_only:
                    pipe.ctx.set_robust(None) if setting is None else pipe.ctx.set_robust(**setting)
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
                res[label]["solve_ms"].append(round(prof["solve"][0] / steps, 4)); res[label]["step_ms"].append(round(dt / steps * 1e3, 4))
                if "v_err_object" not in res[label]:
                    rec = pipe.ctx.pairs_download(points=False)["records"]
                    err = np.linalg.norm(rec[:, :3] - np.asarray(p0["v"]), axis=1) / np.linalg.norm(p0["v"])
                    res[label].update(v_err_object=round(float(np.median(err[1::2])), 4), v_err_plain_scene=round(float(np.median(err[0::2])), 4))
    finally:
        if not off_only:
            pipe.ctx.set_robust(None)
        pipe.close()
    for r in res.values():
        r["solve_ms_median"] = float(np.median(r["solve_ms"])); r["step_ms_median"] = float(np.median(r["step_ms"]))
        r["step_ms_spread"] = round(float(max(r["step_ms"]) - min(r["step_ms"])), 4)
    line = dict(config=name, frame=f"{w}x{h}", pairs_per_step=batch, slices=S["streams"], steps=steps, rounds=rounds, variants=res)
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="both", choices=["c1", "c2", "both"])
    ap.add_argument("--batch", type=int, default=0, help="pairs per step (default: the configuration's)")
    ap.add_argument("--steps", type=int, default=20, help="queued steps per measurement (>= 20)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--off-only", action="store_true", help="measure the plain path alone (also runs on a commit without the setting)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust_bench.json"))
    args = ap.parse_args()
    load_package()
    lines = [run(c, args.batch, max(20, args.steps), args.rounds, args.off_only) for c in (("c1", "c2") if args.config == "both" else (args.config,))]
    with open(args.out, "w") as f:
        json.dump({"_note": "tools/bench_robust.py on one MI355X: solve stage (device events) and whole step (wall clock over queued steps) per "
                            "variant, alternated in one process; v_err_*: median relative velocity error of the pairs with / without a moving object",
                   "results": lines}, f, indent=1)


if __name__ == "__main__":
    main()
