"""The loop of velocity_measurment_node:92-177 (commented-out blocks restored) written once with the CPU oracle's functions
(NodeLoop): the checker the video-stream GPU tests compare `FlowStream` against, frame by frame.  What varies between the device's
stream steps goes in as a plug: the tracker (tests/lk_seed_reference.py for seeded LK), the solver (tests/robust_stream_oracle.py
for the robust solve), the motion source (sensor row or IMU state) and the filter.  Test infrastructure only."""
import numpy as np

from oracle import image_oracle as io, estimation_oracle as eo


def disc_mask(h, w, pts, radius):
    m = np.ones((h, w), np.uint8)
    for x, y in pts:
        cx, cy = int(x), int(y)
        y0, y1 = max(0, cy - radius), min(h, cy + radius + 1); x0, x1 = max(0, cx - radius), min(w, cx + radius + 1)
        if y0 < y1 and x0 < x1:
            yy, xx = np.ogrid[y0:y1, x0:x1]
            m[y0:y1, x0:x1][(yy - cy) ** 2 + (xx - cx) ** 2 <= radius * radius] = 0
    return m


def imu_messages(rng, t0, n, tilt=0.02, rate=(0, 0, 0), rate_sigma=0.002):
    """n IMU messages [n,15] 20 ms apart from time t0 (seconds): a slightly tilted vehicle turning at `rate` on average."""
    out = np.zeros((n, 15))
    for k in range(n):
        t = t0 + 0.02 * (k + 1)
        ax = rng.normal(0, tilt, 3)
        q = np.array([ax[0] / 2, ax[1] / 2, ax[2] / 2, 1.0]); q /= np.linalg.norm(q)
        out[k] = [int(t), int((t - int(t)) * 1e9), *q, *(np.asarray(rate) + rng.normal(0, rate_sigma, 3)), 1e-4, 2e-4, 3e-4,
                  *(rng.normal(0, 0.05, 3) + [0, 0, 9.81])]
    return out


def default_lk(cfg):
    """The tracker plug lk(g_prev, g, old) -> (next, status, err): the oracle's LK with the config's parameters."""
    return lambda g_prev, g, old: io.lk_pyr(g_prev, g, old, cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr)


def track(lk, g_prev, g, old):
    """-> (next [n,2] f32, status [n] u8), empty without tracks."""
    if not len(old):
        return np.zeros((0, 2), np.float32), np.zeros(0, np.uint8)
    new, st, _ = lk(g_prev, g, old)
    return new.reshape(-1, 2), st.ravel().astype(np.uint8)       # cv2 hands out uint8 (of_module.py:93)


def plain_solve(x, u, ok, d, nrm, om):
    """The solver plug solve(all points, all flows, status mask, d, normal, omega) -> dict(v or None, solved, keep = the points that
    stay tracks, extras): solve_lgs on the tracked points (node:257) once there are 3 of them; every tracked point stays."""
    solved = int(ok.sum()) >= 3
    return dict(v=eo.solve_lgs_node(x[ok], u[ok], d, nrm, om)[0] if solved else None, solved=solved, keep=ok)


class NodeLoop:
    """node:117-175 (restored) for one stream, one frame per step().  Construction = goodFeaturesToTrack on the first frame.
    lk, solve: the plugs above (lk also per step: a seeded tracker is a new closure every frame).
    imu_offset: None = R, normal, omega and the lever arm come from the step's sensor row (include/ofk.h: 7..15, 1..3, 4..6, 16..18);
    a lever arm = they come from the dead-reckoning state that call_imu (node:61-89) keeps over the step's messages.
    model (pipeline.FilterModel): predict with the velocity increments of those messages on every step, correct with +v_uav, the gps
    row stacked under it when given, on a solved one.  overwrite: without a model a solved step sets self.vel = v_uav (node:261).
    step() returns dict(v, v_uav, x, P, vel, tracks, n_old, n_tracked, solved, keep, the solver's extras)."""

    def __init__(self, first_frame, cfg, min_feat, radius, lk=None, solve=plain_solve, imu_offset=None, model=None, overwrite=False):
        self.cfg, self.min_feat, self.radius, self.lk, self.solve = cfg, min_feat, radius, lk or default_lk(cfg), solve
        self.g_prev = io.gray_bgr8(first_frame)
        self.tracks = io.good_features(self.g_prev, cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size).reshape(-1, 2)
        self.imu = self.x = self.P = None
        if imu_offset is not None:
            self.offset = np.asarray(imu_offset, np.float64)
            self.imu = dict(vel=np.array([0.1, 0.1, 0.1]), old_time=0.0, time_zero=0.0, first=True, rotation=np.eye(3),
                            normal=np.array([0.0, 0, 1]), ang=np.zeros(3))                   # node:182-217
        self.model, self.overwrite = model, overwrite
        if model is not None:
            self.x, self.P = np.array(model.x0, np.float64), np.array(model.P0, np.float64)

    def step(self, frame, sr, msgs=(), gps=None, lk=None):
        cfg, model = self.cfg, self.model
        dv = np.zeros(3)
        if self.imu is None:
            R, nrm, om, offset = sr[7:16].reshape(3, 3), sr[1:4], sr[4:7], sr[16:19]
        else:
            for m in np.asarray(msgs, np.float64).reshape(-1, 15):
                v0 = self.imu["vel"].copy()
                self.imu = eo.imu_step(self.imu, m[0], m[1], m[2:6], m[6:9], m[9:12], m[12:15])
                dv += self.imu["vel"] - v0
            R, nrm, om, offset = self.imu["rotation"], self.imu["normal"], self.imu["ang"], self.offset
        g = io.gray_bgr8(frame)
        old = self.tracks; n_old = len(old)
        new, st = track(lk or self.lk, self.g_prev, g, old)                                  # :133
        ok = st == 1
        x = (new.astype(np.float64) - [sr[20], sr[21]]) * sr[19]; u = (new.astype(np.float64) - old) * sr[19]     # :229-235
        if model is not None:
            self.x, self.P = eo.kf_predict(self.x, self.P, model.F, model.Q, model.B, dv)
        out = self.solve(x, u, ok, sr[0], nrm, om)
        vu = None if out["v"] is None else eo.post_solve(out["v"], R, om, offset)           # lever arm + rotation (:258)
        if out["solved"] and model is not None:
            self.x, self.P = eo.kf_correct(self.x, self.P, model.H, model.R, vu if gps is None else np.concatenate([vu, np.asarray(gps, np.float64)]))
        elif out["solved"] and self.overwrite:
            self.imu["vel"] = vu.copy()
        self.tracks = new[out["keep"]]
        if n_old <= self.min_feat and cfg.max_corners - n_old > 0:                           # :160-172, against the previous frame
            mask = disc_mask(*g.shape, old, self.radius)
            newf = io.good_features(self.g_prev, cfg.max_corners - n_old, cfg.quality, cfg.min_distance, cfg.block_size, mask=mask).reshape(-1, 2)
            self.tracks = np.concatenate([self.tracks, newf])[:cfg.max_corners]
        self.g_prev = g
        return dict(out, v_uav=vu, x=None if model is None else self.x.copy(), P=None if model is None else self.P.copy(),
                    vel=None if self.imu is None else self.imu["vel"].copy(), tracks=self.tracks.copy(), n_old=n_old, n_tracked=int(ok.sum()))


def oracle_stream(frames, cfg, sensors, min_feat, radius):
    """The plain FlowStream.step: returns per step (v_obs or None, tracks after the step, n_old, n_tracked)."""
    loop = NodeLoop(frames[0], cfg, min_feat, radius)
    first = loop.tracks.copy()
    steps = [loop.step(frames[t], sensors) for t in range(1, len(frames))]
    return first, [(o["v"], o["tracks"], o["n_old"], o["n_tracked"]) for o in steps]


def oracle_node_fused(frames, cfg, statics, imu_msgs, min_feat, radius, model=None, gps=None):
    """The loop with the node's IMU callback in it: self.vel = v_uav (node:261) or, with `model` (pipeline.FilterModel.ekf6; gps rows
    for ekf6(gps=True)), the filter.  statics = dict(d, offset, scaling, cx, cy).  imu_msgs[t-1] = messages [M,15] before frame t.
    Returns per step (v_obs, v_uav, velocity state after the step (IMU vel or filter x), tracks, n_old, n_tracked)."""
    sr = np.zeros(22)
    sr[0] = statics["d"]; sr[19:22] = statics["scaling"], statics["cx"], statics["cy"]
    loop = NodeLoop(frames[0], cfg, min_feat, radius, imu_offset=statics["offset"], model=model, overwrite=model is None)
    first = loop.tracks.copy()
    steps = [loop.step(frames[t], sr, imu_msgs[t - 1], None if gps is None else gps[t - 1]) for t in range(1, len(frames))]
    return first, [(o["v"], o["v_uav"], o["vel"] if model is None else o["x"], o["tracks"], o["n_old"], o["n_tracked"]) for o in steps]


def oracle_of_module(frames, cfg, normal, controls, omegas, min_feat, cx, cy, model, synthetic_flow=True, hold=False):
    """optical_flow_experiments/of_module.py:78-167 written with the oracle's functions, one stream:
    re-detect (replace) when <= min_feat tracks (:83-86) -> LK (:88) -> x = [new - pix_trans, 1] in pixels (:96-102) -> u = LK flow or
    the synthetic rotational field of omega on the un-centred positions (:107-114) -> kalman.predict(control) (:122) -> legacy
    r_tilde with the predicted velocity (:125) -> keep r - (status - 1) >= T with uint8 status, i.e. tracked and r >= T (:129-131) -> A_i = [p]x / dist_i system, lstsq
    (:136-146) -> kalman.correct(-v_obs) (:152) -> old_pos = new_pos[keep] (:166).
    On <= 3 feasible points the script `continue`s without advancing the frame (:138): hold=True does the same (the device's
    ofk_fusion.hold_on_skip, one stream per context); hold=False advances the frame and lets the filter keep its prediction, which
    is what a batch of streams sharing one frame swap does (include/ofk.h, ofk_stream_step_fused).
    Returns per step (v_obs or None, filter state x, P, tracks after the step, n_old, n_kept)."""
    n = np.asarray(normal, np.float64); lk = default_lk(cfg)
    g_prev = io.gray_bgr8(frames[0])
    old = io.good_features(g_prev, cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size).reshape(-1, 2)
    first = old.copy()
    xk, P = np.array(model.x0, np.float64), np.array(model.P0, np.float64)
    steps = []
    for t in range(1, len(frames)):
        g = io.gray_bgr8(frames[t])
        if len(old) <= min_feat:
            k = cfg.max_corners - len(old)
            old = io.good_features(g_prev, k, cfg.quality, cfg.min_distance, cfg.block_size).reshape(-1, 2) if k > 0 else np.zeros((0, 2), np.float32)
        n_old = len(old)
        new, st = track(lk, g_prev, g, old)
        X = new[:, 0].astype(np.float64); Y = new[:, 1].astype(np.float64)
        x3 = np.stack([X - cx, Y - cy, np.ones_like(X)], 1)
        w = np.asarray(omegas[t - 1], np.float64)
        if synthetic_flow:
            u3 = np.stack([X * Y * w[0] + (1 + X ** 2) * w[1] - Y * w[2], -(1 + Y ** 2) * w[0] + X * Y * w[1] + X * w[2], np.zeros_like(X)], 1)
        else:
            u3 = np.concatenate([new.astype(np.float64) - old.astype(np.float64), np.zeros((n_old, 1))], 1)
        xk, P = eo.kf_predict(xk, P, model.F, model.Q, model.B, np.asarray(controls[t - 1], np.float64))
        with np.errstate(divide="ignore", invalid="ignore"):
            r, dist = eo.r_tilde_legacy(x3, u3, n, xk[:3]) if n_old else (np.zeros(0), np.zeros(0))
            keep = (r - (st - np.uint8(1))) >= cfg.feas_T           # of_module.py:129 as written: uint8 status-1 wraps to 255 for a lost point
        v = None
        if keep.sum() > 3:
            v = eo.solve_of_module(x3[keep], u3[keep], dist[keep], n)[0]
            xk, P = eo.kf_correct(xk, P, model.H, model.R, -v)
        elif hold:                                               # of_module.py:138 `continue`: old_gray and old_pos stay as they are
            steps.append((None, xk.copy(), P.copy(), old.copy(), n_old, int(keep.sum())))
            continue
        old = new[keep]
        steps.append((v, xk.copy(), P.copy(), old.copy(), n_old, int(keep.sum())))
        g_prev = g
    return first, steps
