"""The robust solve (tests/robust_reference.py) as the solver of the video-stream loop (tests/stream_oracle.py::NodeLoop), as the
device's stream steps run it under ofk_set_robust: FlowStream.step, step_fused on the sensors, and step_fused on the resident IMU
state with the 6-state filter.  With `drop` the points whose final weight is 0 leave the tracks like points that lost their status.
And the scene it is used with.  Test infrastructure only.

The scene: synth.render_sequence with a textured rectangle of OBJECT_SIZE pasted into frame t at OBJECT_AT + t * OBJECT_STEP - an
object that crosses the view on its own.  What `drop` achieves is stated on this loop (tests/test_robust_reference.py): the share of
the tracks that lie on the object after the last frame, per stream (seeds 900, 901), measured with the committed code:
    drop off 0.092, 0.122     drop on 0.000, 0.000"""
import numpy as np

import robust_reference as rr

OBJECT_SIZE = (160, 220)
OBJECT_AT = np.array([60, 200])                                  # row, column in frame 0
OBJECT_STEP = np.array([5, -7])                                  # rows, columns per frame
MOTION = dict(v=(0.004, -0.003, 0.002), omega=(0.003, -0.002, 0.004), d=1.0)
SETTING = dict(loss=rr.TUKEY, c=4.685, iters=5, hypotheses=64, seed=0x1234ABCD5678)


def sequence(synth, h, w, seed, n_frames):
    """(frames with the object pasted in, info)"""
    frames, info = synth.render_sequence(h, w, seed, n_frames, margin=200, **MOTION)
    frames = frames.copy()
    oh, ow = OBJECT_SIZE
    tex = synth.render_pair(oh + 40, ow + 40, seed + 100, margin=96)["prev"][20:20 + oh, 20:20 + ow]
    for t in range(n_frames):
        r, c = OBJECT_AT + t * OBJECT_STEP
        frames[t, r:r + oh, c:c + ow] = tex
    return frames, info


def on_object(pts, t):
    r, c = OBJECT_AT + t * OBJECT_STEP
    return rr.on_object(pts, OBJECT_SIZE, row=r, col=c)


def robust_solver(problem, drop, fused, setting=SETTING):
    """stream_oracle.NodeLoop's solver plug for a stream under ofk_set_robust.  problem: the stream's index in the batch (it picks the
    sample).  fused: step_fused solves with more than min_solve = 2 kept points, the plain stream step whenever one is kept.
    Extras of the step's record: used, weights, stats, rank, gap, near, rss."""
    min_cnt = 2 if fused else 0

    def solve(x, u, ok, d, nrm, om):
        r = rr.robust_solve(rr.NODE, x, u, d, nrm, om, valid=ok, problem=problem, min_cnt=min_cnt, **setting)
        return dict(v=r["v"], solved=int(ok.sum()) > min_cnt, keep=ok & (r["weights"] > 0) if drop else ok,
                    used=r["cnt"], weights=r["weights"], stats=r["stats"], rank=r["rank"], gap=r["gap"], near=r["near"], rss=r["r"])
    return solve
