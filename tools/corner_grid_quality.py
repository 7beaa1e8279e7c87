#!/usr/bin/env python3
"""What the corner grid buys, on the CPU (oracle and reference only; no device).

  1. The concentrated-contrast scene: 640x480 band-limited noise at amplitude 12 with a 200x230 box of amplitude 55 (15 % of the
     frame), maxCorners 300, quality 0.01, minDistance 10, block 7: the share of the corners inside the box, plain against a grid of
     64-pixel cells holding at most 4 corners.
  2. The moving-object scenes of tests/robust_reference.py (a textured rectangle that moves on its own), with the object's contrast
     raised and the ground's lowered (`--object-gain`, `--ground-gain` about mid-gray) so that the plain selection crowds onto the
     object: share of the tracked corners on the object and relative error |v_obs - v| / |v| of the node's least squares and of the
     robust solve (TUKEY, 64 hypotheses, 5 rounds), plain against the grid, over the scenes' seeds.

  python tools/corner_grid_quality.py [--cell 64] [--cap 4] [--object-gain 1.6] [--ground-gain 0.35]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package  # noqa: E402


def gain_about_gray(img, g):
    return np.clip(128.0 + g * (img.astype(np.float64) - 128.0), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cell", type=int, default=64); ap.add_argument("--cap", type=int, default=4)
    ap.add_argument("--object-gain", type=float, default=1.6); ap.add_argument("--ground-gain", type=float, default=0.35)
    args = ap.parse_args()
    load_package()
    from of_amd import synth
    from oracle import image_oracle as io, estimation_oracle as eo
    import corner_grid_cases as K, corner_grid_reference as R, robust_reference as rr
    grid = (args.cell, args.cap, 0)
    q = K.QUALITY_SCENE
    e = K.eig_of("quality", q["block"])
    y0, x0, bh, bw = q["box"]
    out = {"concentrated": {}}
    for label, g in (("plain", R.OFF), ("grid", grid)):
        p, st, _ = R.select(e, q["max_corners"], q["quality"], q["min_distance"], grid=g)
        inside = (p[:, 0] >= x0) & (p[:, 0] < x0 + bw) & (p[:, 1] >= y0) & (p[:, 1] < y0 + bh)
        out["concentrated"][label] = dict(corners=st[0], examined=st[1], share_on_object=round(float(inside.mean()), 3))
    out["moving_object"] = {}
    for size in rr.OBJECT_SIZES:
        rows = {k: dict(share=[], node=[], robust=[]) for k in ("plain", "grid")}
        for seed in rr.SCENE_SEEDS:
            pair, prev, nxt = rr.scene(synth, seed, size)
            oh, ow = size
            m0 = np.zeros(prev.shape[:2], bool); m0[60:60 + oh, 80:80 + ow] = True
            m1 = np.zeros(prev.shape[:2], bool); m1[65:65 + oh, 73:73 + ow] = True
            prev = np.where(m0[..., None], gain_about_gray(prev, args.object_gain), gain_about_gray(prev, args.ground_gain))
            nxt = np.where(m1[..., None], gain_about_gray(nxt, args.object_gain), gain_about_gray(nxt, args.ground_gain))
            g0, g1 = io.gray_bgr8(prev), io.gray_bgr8(nxt)
            for label, g in (("plain", R.OFF), ("grid", grid)):
                pts = R.good_features(g0, 300, 0.01, 10, 7, grid=g)[0]
                n, s, _ = io.lk_pyr(g0, g1, pts.reshape(-1, 1, 2), 15, 3, 20, 0.03, 1e-4)
                ok = s.ravel() == 1
                new = n.reshape(-1, 2).astype(np.float64); old = pts.astype(np.float64)
                x = (new - [pair["cx"], pair["cy"]]) * pair["scaling"]; u = (new - old) * pair["scaling"]
                vp = eo.solve_lgs_node(x[ok], u[ok], pair["d"], pair["n"], pair["omega"])[0]
                r = rr.robust_solve(rr.NODE, x, u, pair["d"], pair["n"], pair["omega"], valid=ok, **rr.EXPERIMENT)
                rows[label]["share"].append(float((rr.on_object(old, size) & ok).sum() / max(1, ok.sum())))
                rows[label]["node"].append(rr.rel_err(vp, pair["v"])); rows[label]["robust"].append(rr.rel_err(r["v"], pair["v"]))
        out["moving_object"]["%dx%d" % size] = {k: {m: dict(min=round(min(v), 4), median=round(float(np.median(v)), 4), max=round(max(v), 4))
                                                        for m, v in d.items()} for k, d in rows.items()}
    print(json.dumps(dict(grid=dict(cell=args.cell, cap=args.cap), object_gain=args.object_gain, ground_gain=args.ground_gain, **out), indent=1))


if __name__ == "__main__":
    main()
