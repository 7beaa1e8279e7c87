#!/usr/bin/env python3
"""What the track gates (ofk_set_track_gate) cost on the device, at the shapes of bench.py's configs c1 (1080p, 500 corners,
512 pairs, one slice) and c2 (640x480, 500 corners, 1024 pairs, two slices).

Settings: off (the default path), plain backward pass at the forward depth, seeded backward pass at depths 3 / 1 / 0, and the err cap
alone (at the median err of the ungated run's tracked points) - alternated inside one process, `--rounds` times each.  Per setting
and round: the LK stage in milliseconds per step (ofk_profile_*: device events around the stage, which holds the backward pass and
the gate kernel) and the whole step (wall clock around `--steps` queued steps between two syncs).  Per setting once: the kept share
(status 1 behind the gate over the detected corners), the gate's four counts summed over the batch, and the share of wrong points
among the kept ones on the rendered pairs (status 1 and more than 0.5 px from synth.true_flow_px).
Frames: synth.make_batch; sensors: the pairs' true motion.

  python tools/bench_track_gate.py [--config c1|c2|both] [--motion default|yaw0.08|...] [--batch N] [--out profiles/track_gate_bench.json]
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
    "yaw0.15": dict(v=(0.003, -0.002, 0.001), omega=(0.002, -0.001, 0.15)),
}
FB_THR = 0.5
# label, track_gate_setting's keywords (err_max None = the median err of the ungated run)
SETTINGS = (("off", None), ("plain L3", dict(fb="plain", fb_level=-1)), ("seeded L3", dict(fb="seeded", fb_level=3)),
            ("seeded L1", dict(fb="seeded", fb_level=1)), ("seeded L0", dict(fb="seeded", fb_level=0)), ("err cap", dict(err_max=None)))


def wrong_share(out, base):
    """(kept points more than 0.5 px from the true end point, kept points) over the rendered pairs."""
    from of_amd import synth
    wrong = kept = 0
    for b, pair in enumerate(base):
        n = int(out["counts"][b])
        p = out["prev_pts"][b, :n].astype(np.float64)
        d = np.linalg.norm(out["next_pts"][b, :n].astype(np.float64) - (p + synth.true_flow_px(pair["H"], p)), axis=1)
        k = out["status"][b, :n] == 1
        wrong += int(np.sum(k & (d > 0.5))); kept += int(k.sum())
    return wrong, kept


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
    cfg = PipelineConfig(max_corners=S["corners"], quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)
    params = cfg.to_params()
    pipe = FlowPipeline(w, h, batch, cfg, streams=S["streams"])
    res = {s[0]: dict(lk_ms=[], step_ms=[]) for s in SETTINGS}
    try:
        pipe.upload(prev, nxt, sensors)
        ungated = pipe.run()
        used = np.arange(ungated["status"].shape[1])[None, :] < ungated["counts"][:, None]
        cap = float(np.median(ungated["err"][used & (ungated["status"] == 1)]))
        for _ in range(rounds):
            for label, kw in SETTINGS:
                if kw is None:
                    pipe.ctx.set_track_gate(None)
                else:
                    kw = dict(kw, fb_thr=FB_THR)
                    if "err_max" in kw:
                        kw["err_max"] = cap
                    pipe.ctx.set_track_gate(**kw)
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
                if "kept_share" not in res[label]:
                    out = pipe.ctx.pairs_download()
                    corners = int(out["counts"].sum())
                    kept = int(sum(int((out["status"][b, :out["counts"][b]] == 1).sum()) for b in range(batch)))
                    wr, kp = wrong_share(out, base)
                    res[label].update(kept_share=round(kept / max(1, corners), 4), corners_mean=round(corners / batch, 2),
                                      wrong_among_kept=round(wr / max(1, kp), 4), setting=kw,
                                      v_err=[round(float(np.linalg.norm(out["records"][b, :3] - base[b]["v"])), 5) for b in range(len(base))])
                    if kw is not None:
                        res[label]["stats_sum"] = [int(x) for x in pipe.track_gate_stats().sum(0)]
    finally:
        pipe.ctx.set_track_gate(None)
        pipe.close()
    for r in res.values():
        r["lk_ms_median"] = float(np.median(r["lk_ms"])); r["step_ms_median"] = float(np.median(r["step_ms"]))
    line = dict(config=name, frame=f"{w}x{h}", pairs_per_step=batch, slices=S["streams"], motion=motion, steps=steps, rounds=rounds, fb_thr=FB_THR,
                settings=res)
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="both", choices=["c1", "c2", "both"])
    ap.add_argument("--motion", default="default,yaw0.08", help="comma-separated: " + ", ".join(MOTIONS))
    ap.add_argument("--batch", type=int, default=0, help="pairs per step (default: the configuration's)")
    ap.add_argument("--steps", type=int, default=20, help="queued steps per measurement (>= 20)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_gate_bench.json"))
    args = ap.parse_args()
    load_package()
    lines = [run(c, m, args.batch, max(20, args.steps), args.rounds) for c in (("c1", "c2") if args.config == "both" else (args.config,))
             for m in args.motion.split(",")]
    with open(args.out, "w") as f:
        json.dump({"_note": "tools/bench_track_gate.py on one MI355X: LK stage (device events; backward pass and gate kernel included) and whole step "
                            "(wall clock over queued steps) per setting, alternated in one process; kept_share = status 1 behind the gate over the "
                            "detected corners; wrong_among_kept = kept points more than 0.5 px from the true flow, on the rendered pairs",
                   "results": lines}, f, indent=1)


if __name__ == "__main__":
    main()
