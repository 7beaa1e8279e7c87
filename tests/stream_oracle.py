"""The loop of velocity_measurment_node:92-177 (commented-out blocks restored) written once with the CPU oracle's functions
(NodeLoop): the checker the video-stream GPU tests compare `FlowStream` against, frame by frame.  What varies between the device's
stream steps goes in as a plug: the tracker (tests/lk_seed_reference.py for seeded LK, tests/track_gate_reference.py for the gates and
for both together), the solver (tests/robust_stream_oracle.py for the robust solve), the detection (tests/corner_grid_reference.py
for the corner grid), the exclusion zones (tests/zones_reference.py), the motion source (sensor row or IMU state) and the filter;
the plugs compose.  Test infrastructure only."""
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


def default_detect(cfg):
    """The detection plug detect(gray, budget, mask, occ_pts) -> points [n,2] f32: goodFeaturesToTrack with the config's parameters.
    occ_pts (the old tracks of an append-mode re-detection, None elsewhere) is the corner grid's occupancy list: unused here."""
    return lambda gray, budget, mask, occ_pts: io.good_features(gray, budget, cfg.quality, cfg.min_distance, cfg.block_size, mask=mask).reshape(-1, 2)


def feasibility_solve(v_prior, feas_T, min_cnt=2):
    """The solver plug of a stream step with p->use_feasibility (node:238-245): the tracked points with r_tilde <= feas_T against the
    prior velocity stay, solve_lgs on them when there are more than min_cnt (ofk_fusion.min_solve; the plain step: 0)."""
    def solve(x, u, ok, d, nrm, om):
        keep = np.array(ok, bool)
        if len(x):
            with np.errstate(all="ignore"):
                keep &= eo.r_tilde(x, u, nrm, np.asarray(v_prior, np.float64), d)[0] <= feas_T
        solved = int(keep.sum()) > min_cnt
        return dict(v=eo.solve_lgs_node(x[keep], u[keep], d, nrm, om)[0] if solved else None, solved=solved, keep=keep, used=int(keep.sum()))
    return solve


class NodeLoop:
    """node:117-175 (restored) for one stream, one frame per step().  Construction = the first detection on the first frame.
    lk, solve: the plugs above (lk also per step: a seeded tracker is a new closure every frame).
    lk_src: a tracker plug lk(g_prev, g, old, src) that also takes the sensor row as the step's motion source sees it - normal, omega
    and the prior velocity (22..24) replaced by the IMU state's under imu_offset - which is what a seeded tracker predicts from
    (tests/track_gate_reference.seeded_gated_lk); step(src=) puts a caller's row in the place of the loop's own.
    detect: the detection plug (default_detect), used for the first detection (no mask, no occupancy) and every re-detection.
    imu_offset: None = R, normal, omega and the lever arm come from the step's sensor row (include/ofk.h: 7..15, 1..3, 4..6, 16..18);
    a lever arm = they come from the dead-reckoning state that call_imu (node:61-89) keeps over the step's messages.
    model (pipeline.FilterModel): predict with the velocity increments of those messages on every step, correct with +v_uav, the gps
    row stacked under it when given, on a solved one.  overwrite: without a model a solved step sets self.vel = v_uav (node:261).
    zones: a setting dict (tests/zones_reference.DEFAULT's keys) switches the exclusion zones on: self.table (zones_reference.Table)
    is updated behind the solve from the tracker's status and the solver's keep, rendered into the re-detection's mask and aged at the
    end of the step (include/ofk.h, ofk_zones, rules 1-7).
    replace: the re-detection of ofk_fusion.redetect_replace instead of the node's - before tracking, a stream with few tracks replaces
    them by fresh corners of its previous frame, found without a mask or, with zones, behind a mask of the zones alone; nothing is
    appended behind the solve.
    step() returns dict(v, v_uav, x, P, vel, tracks, n_old, n_tracked, solved, keep, the solver's extras; old, new, status = the
    tracker's points; motion = (R, normal, omega, offset) and dv as the step used them; redetected; with zones: zones = a copy of
    the table behind the step, zones_masked = live zones rendered into the re-detection's mask)."""

    def __init__(self, first_frame, cfg, min_feat, radius, lk=None, solve=plain_solve, imu_offset=None, model=None, overwrite=False,
                 detect=None, zones=None, replace=False, lk_src=None):
        self.cfg, self.min_feat, self.radius, self.lk, self.solve = cfg, min_feat, radius, lk or default_lk(cfg), solve
        self.detect, self.replace, self.lk_src = detect or default_detect(cfg), replace, lk_src
        self.g_prev = io.gray_bgr8(first_frame)
        self.tracks = np.asarray(self.detect(self.g_prev, cfg.max_corners, None, None), np.float32).reshape(-1, 2)
        self.imu = self.x = self.P = None
        if imu_offset is not None:
            self.offset = np.asarray(imu_offset, np.float64)
            self.imu = dict(vel=np.array([0.1, 0.1, 0.1]), old_time=0.0, time_zero=0.0, first=True, rotation=np.eye(3),
                            normal=np.array([0.0, 0, 1]), ang=np.zeros(3))                   # node:182-217
        self.model, self.overwrite = model, overwrite
        if model is not None:
            self.x, self.P = np.array(model.x0, np.float64), np.array(model.P0, np.float64)
        self.setting = self.table = None
        if zones is not None:
            import zones_reference as zr                         # tests/zones_reference.py (it imports this module)
            self.zr, self.setting, self.table = zr, dict(zr.DEFAULT, **zones), zr.Table()

    def _redetect(self, g_old, budget, mask, occ_pts, out):
        """One re-detection on the previous frame behind `mask` (None: none) with the live zones zeroed in it."""
        if self.table is not None:
            out["zones_masked"] = len(self.table.live())
            mask = self.zr.render(self.table, self.setting, np.ones(g_old.shape, np.uint8) if mask is None else mask)
        return np.asarray(self.detect(g_old, budget, mask, occ_pts), np.float32).reshape(-1, 2)

    def step(self, frame, sr, msgs=(), gps=None, lk=None, src=None):
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
        g, g_old = io.gray_bgr8(frame), self.g_prev
        extra = dict(zones_masked=0)
        budget = cfg.max_corners - len(self.tracks)
        redetected = bool(len(self.tracks) <= self.min_feat and budget > 0)
        if self.replace and redetected:                                                      # of_module.py:83-86
            self.tracks = self._redetect(g_old, budget, None, None, extra)
        old = self.tracks; n_old = len(old)
        tracker = lk or self.lk
        if lk is None and self.lk_src is not None:
            if src is None:
                src = np.array(sr, np.float64)
                if self.imu is not None:
                    src[1:4], src[4:7], src[22:25] = nrm, om, self.imu["vel"]
            row = src
            tracker = lambda a, b, o: self.lk_src(a, b, o, row)
        new, st = track(tracker, g_old, g, old)                                              # :133
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
        if self.table is not None:                                                           # rules 1-4: tracked, not kept by the solve stage
            self.zr.update(self.table, self.setting, old, new, st, np.asarray(out["keep"]).astype(np.uint8))
        self.tracks = new[out["keep"]]
        if redetected and not self.replace:                                                  # :160-172, against the previous frame
            newf = self._redetect(g_old, budget, disc_mask(*g.shape, old, self.radius), old, extra)
            self.tracks = np.concatenate([self.tracks, newf])[:cfg.max_corners]
        if self.table is not None:
            self.zr.age(self.table)                                                          # rule 7
            extra["zones"] = self.table.copy()
        self.g_prev = g
        return dict(out, v_uav=vu, x=None if model is None else self.x.copy(), P=None if model is None else self.P.copy(),
                    vel=None if self.imu is None else self.imu["vel"].copy(), tracks=self.tracks.copy(), n_old=n_old, n_tracked=int(ok.sum()),
                    old=old.copy(), new=new, status=st, motion=(np.array(R, np.float64), np.array(nrm, np.float64), np.array(om, np.float64),
                    np.array(offset, np.float64)), dv=dv, redetected=redetected, **extra)


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


def oracle_of_module(frames, cfg, normal, controls, omegas, min_feat, cx, cy, model, synthetic_flow=True, hold=False, detect=None, zones=None):
    """optical_flow_experiments/of_module.py:78-167 written with the oracle's functions, one stream:
    re-detect (replace) when <= min_feat tracks (:83-86) -> LK (:88) -> x = [new - pix_trans, 1] in pixels (:96-102) -> u = LK flow or
    the synthetic rotational field of omega on the un-centred positions (:107-114) -> kalman.predict(control) (:122) -> legacy
    r_tilde with the predicted velocity (:125) -> keep r - (status - 1) >= T with uint8 status, i.e. tracked and r >= T (:129-131) -> A_i = [p]x / dist_i system, lstsq
    (:136-146) -> kalman.correct(-v_obs) (:152) -> old_pos = new_pos[keep] (:166).
    On <= 3 feasible points the script `continue`s without advancing the frame (:138): hold=True does the same (the device's
    ofk_fusion.hold_on_skip, one stream per context); hold=False advances the frame and lets the filter keep its prediction, which
    is what a batch of streams sharing one frame swap does (include/ofk.h, ofk_stream_step_fused).
    detect: NodeLoop's detection plug (default_detect), for the first detection and the replacing one.
    zones: a setting dict (tests/zones_reference.DEFAULT's keys) switches the exclusion zones on (include/ofk.h, ofk_zones): the
    replacing detection runs behind a mask of the zones alone, the rejects are the tracked points (status 1) the legacy keep refused,
    and a held step touches neither the table nor its age.
    Returns per step (v_obs or None, filter state x, P, tracks after the step, n_old, n_kept), with zones a seventh entry
    dict(zones = a copy of the table behind the step, rejects, redetected, zones_masked, held)."""
    n = np.asarray(normal, np.float64); lk = default_lk(cfg)
    detect = detect or default_detect(cfg)
    table = None
    if zones is not None:
        import zones_reference as zr                             # tests/zones_reference.py (it imports this module)
        setting, table = dict(zr.DEFAULT, **zones), zr.Table()
    g_prev = io.gray_bgr8(frames[0])
    old = np.asarray(detect(g_prev, cfg.max_corners, None, None), np.float32).reshape(-1, 2)
    first = old.copy()
    xk, P = np.array(model.x0, np.float64), np.array(model.P0, np.float64)
    steps = []
    for t in range(1, len(frames)):
        g = io.gray_bgr8(frames[t])
        info = dict(redetected=False, zones_masked=0, rejects=0, held=False)
        if len(old) <= min_feat:
            k = cfg.max_corners - len(old)
            mask = None
            if table is not None and k > 0:
                info["zones_masked"] = len(table.live())
                mask = zr.render(table, setting, np.ones(g_prev.shape, np.uint8))
            info["redetected"] = k > 0
            old = np.asarray(detect(g_prev, k, mask, None), np.float32).reshape(-1, 2) if k > 0 else np.zeros((0, 2), np.float32)
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
            held = (None, xk.copy(), P.copy(), old.copy(), n_old, int(keep.sum()))
            steps.append(held if table is None else held + (dict(info, zones=table.copy(), held=True),))
            continue
        if table is not None:
            zr.update(table, setting, old, new, st, keep.astype(np.uint8))
            zr.age(table)
            info.update(zones=table.copy(), rejects=int(np.count_nonzero((st == 1) & ~keep)))
        old = new[keep]
        steps.append((v, xk.copy(), P.copy(), old.copy(), n_old, int(keep.sum())) + (() if table is None else (info,)))
        g_prev = g
    return first, steps
