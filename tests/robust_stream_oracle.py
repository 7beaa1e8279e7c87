"""The video-stream loops of tests/stream_oracle.py restated one frame at a time with the robust solve (tests/robust_reference.py) in
the place of the plain one, as the device's stream steps run it under ofk_set_robust: FlowStream.step (node:131-175), step_fused on
the sensors, and step_fused on the resident IMU state with the 6-state filter (oracle_node_fused).  With `drop` the points whose final
weight is 0 leave the tracks like points that lost their status.  Test infrastructure only.

The scene: synth.render_sequence with a textured rectangle of OBJECT_SIZE pasted into frame t at OBJECT_AT + t * OBJECT_STEP - an
object that crosses the view on its own.  What `drop` achieves is stated on this loop (tests/test_robust_reference.py): the share of
the tracks that lie on the object after the last frame, per stream (seeds 900, 901), measured with the committed code:
    drop off 0.092, 0.122     drop on 0.000, 0.000"""
import numpy as np

from oracle import image_oracle as io, estimation_oracle as eo
from stream_oracle import disc_mask
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


class RobustLoop:
    """One stream.  kind "step": the plain stream step (solved whenever a point is kept); "fused": step_fused without filter on the
    sensors' normal / omega (solved with more than min_solve = 2 kept points); "ekf6": step_fused on the IMU state with
    FilterModel.ekf6 (`model`), predict with the velocity increments of the messages, correct with +v_uav of the robust solve.
    step() returns dict(v, v_uav, x, P, tracks, n_old, n_tracked, used, weights, stats)."""

    def __init__(self, first_frame, cfg, min_feat, radius, kind, problem, drop, setting=SETTING, offset=(0.0, 0.0, 0.1), model=None):
        self.cfg, self.min_feat, self.radius, self.kind, self.problem, self.drop, self.setting = cfg, min_feat, radius, kind, problem, drop, setting
        self.h, self.w = first_frame.shape[:2]
        self.g_prev = io.gray_bgr8(first_frame)
        self.tracks = io.good_features(self.g_prev, cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size).reshape(-1, 2)
        self.offset = np.asarray(offset, np.float64)
        self.model = model
        self.state = dict(vel=np.array([0.1, 0.1, 0.1]), old_time=0.0, time_zero=0.0, first=True, rotation=np.eye(3), normal=np.array([0.0, 0, 1]),
                          ang=np.zeros(3))                       # node:182-217
        if model is not None:
            self.x, self.P = np.array(model.x0, np.float64), np.array(model.P0, np.float64)

    def step(self, frame, sr, msgs=None):
        cfg = self.cfg
        dv = np.zeros(3)
        if self.kind == "ekf6":
            for m in np.asarray(msgs, np.float64).reshape(-1, 15):
                v0 = self.state["vel"].copy()
                self.state = eo.imu_step(self.state, m[0], m[1], m[2:6], m[6:9], m[9:12], m[12:15])
                dv += self.state["vel"] - v0
            R, nrm, om = self.state["rotation"], self.state["normal"], self.state["ang"]
        else:
            R, nrm, om = sr[7:16].reshape(3, 3), sr[1:4], sr[4:7]
        g = io.gray_bgr8(frame)
        old = self.tracks; n_old = len(old)
        if n_old:
            new, st, _ = io.lk_pyr(self.g_prev, g, old, cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr)
            new = new.reshape(-1, 2); ok = st.ravel() == 1
        else:
            new = np.zeros((0, 2), np.float32); ok = np.zeros(0, bool)
        x = (new.astype(np.float64) - [sr[20], sr[21]]) * sr[19]; u = (new.astype(np.float64) - old) * sr[19]
        if self.kind == "ekf6":
            self.x, self.P = eo.kf_predict(self.x, self.P, self.model.F, self.model.Q, self.model.B, dv)
        min_cnt = 0 if self.kind == "step" else 2
        r = rr.robust_solve(rr.NODE, x, u, sr[0], nrm, om, valid=ok, problem=self.problem, min_cnt=min_cnt, **self.setting)
        solved = int(ok.sum()) > min_cnt
        vu = eo.post_solve(r["v"], R, om, self.offset if self.kind == "ekf6" else sr[16:19])
        if self.kind == "ekf6" and solved:
            self.x, self.P = eo.kf_correct(self.x, self.P, self.model.H, self.model.R, vu)
        keep = ok & (r["weights"] > 0) if self.drop else ok
        tracked = new[keep]
        if n_old <= self.min_feat and cfg.max_corners - n_old > 0:
            mask = disc_mask(self.h, self.w, old, self.radius)
            newf = io.good_features(self.g_prev, cfg.max_corners - n_old, cfg.quality, cfg.min_distance, cfg.block_size, mask=mask).reshape(-1, 2)
            self.tracks = np.concatenate([tracked, newf])[:cfg.max_corners]
        else:
            self.tracks = tracked
        self.g_prev = g
        return dict(v=r["v"], v_uav=vu, x=None if self.model is None else self.x.copy(), P=None if self.model is None else self.P.copy(),
                    tracks=self.tracks.copy(), n_old=n_old, n_tracked=int(ok.sum()), used=r["cnt"], weights=r["weights"], stats=r["stats"],
                    solved=solved, rank=r["rank"], gap=r["gap"], near=r["near"])
