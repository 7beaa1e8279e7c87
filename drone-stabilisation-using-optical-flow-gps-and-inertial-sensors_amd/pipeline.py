"""pipeline.py — batched, HBM-resident frame-pair pipeline: BGR pair -> gray -> pyramids -> Shi-Tomasi corners
-> pyramidal LK -> centre/scale -> (feasibility) -> least-squares body velocity -> lever arm + rotation.

It strings together, for a batch of independent frame pairs, exactly the stage order of the reference's
offline prototype (optical_flow_experiments/of_module.py:36-152) and of the node's main loop
(velocity_measurment_node:226-261), every stage a HIP kernel (libofk.so, ofk_pairs_run).
"""
from dataclasses import dataclass

import numpy as np

try:
    from . import ofk
except ImportError:      # package directory put on sys.path directly
    import ofk


@dataclass
class CameraModel:
    """The camera of a pipeline (ofk.h: ofk_set_camera): the camera matrix, the lens coefficients in cv2's order ("brown": k1 k2 p1 p2
    [k3 [k4 k5 k6]]; "fisheye": k1..k4) and the ideal pinhole the solve stage is handed: one focal length fo (None = fx) and the centre
    co_x, co_y (None = cx, cy).  iters None = ofk.camera_setting's defaults (20 / 10, not cv2's 5)."""
    fx: float
    fy: float = None
    cx: float = 0.0
    cy: float = 0.0
    k: tuple = ()
    model: str = "brown"
    iters: int = None
    fo: float = None
    co_x: float = None
    co_y: float = None

    def setting(self):
        """The ofk.Camera structure (range-checked)."""
        fo = self.fx if self.fo is None else self.fo
        return ofk.camera_setting(self.model, self.fx, self.fy, self.cx, self.cy, self.k, self.iters, fo, fo, self.co_x, self.co_y)

    def sensor_slots(self):
        """(scaling, cx, cy) for sensors[19..21]: the ideal pinhole's 1 / fo, co_x, co_y."""
        m = self.setting()
        return 1.0 / m.fo_x, m.co_x, m.co_y

    def ideal_radius(self, h, w):
        """The largest ideal normalised radius over the border pixels of the raw h x w frame (the undistort rule of ofk.h on the host,
        float64, the setting's iteration count): what the lens sees at most.  ofk.rectify_setting(r_max=1.05 * cam.ideal_radius(h, w))
        keeps ideal points beyond it, where a Brown polynomial folds back into the frame, out of a rectified view."""
        m = self.setting()
        xs, ys = np.arange(int(w), dtype=np.float64), np.arange(int(h), dtype=np.float64)
        px = np.concatenate([xs, xs, np.zeros(len(ys)), np.full(len(ys), float(w - 1))])
        py = np.concatenate([np.zeros(len(xs)), np.full(len(xs), float(h - 1)), ys, ys])
        x0, y0 = (px - m.cx) / m.fx, (py - m.cy) / m.fy
        k = list(m.k)
        with np.errstate(all="ignore"):
            if m.model == ofk.CAMERA_BROWN:
                k1, k2, p1, p2, k3, k4, k5, k6 = k
                x, y = x0.copy(), y0.copy()
                for _ in range(m.iters):
                    r2 = x * x + y * y
                    icd = (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
                    dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
                    dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
                    x, y = (x0 - dx) * icd, (y0 - dy) * icd
            else:
                k1, k2, k3, k4 = k[:4]
                td = np.sqrt(x0 * x0 + y0 * y0)
                t = td.copy()
                for _ in range(m.iters):
                    t2 = t * t; t4 = t2 * t2; t6 = t4 * t2; t8 = t4 * t4
                    t = t - (t * (1.0 + k1 * t2 + k2 * t4 + k3 * t6 + k4 * t8) - td) / (1.0 + 3.0 * k1 * t2 + 5.0 * k2 * t4 + 7.0 * k3 * t6 + 9.0 * k4 * t8)
                s = np.where(td < 1e-8, 1.0, np.tan(t) / td)
                x, y = x0 * s, y0 * s
            r = float(np.sqrt(x * x + y * y).max())
        if not np.isfinite(r):
            raise ValueError(f"ideal_radius: the undistort iteration of this lens does not stay finite on the border of a {w} x {h} frame "
                             f"(the model does not cover the frame): choose r_max by hand")
        return r


@dataclass
class RollingShutter:
    """The rolling shutter of a pipeline (ofk.h: ofk_set_rolling_shutter): readout = the time from the first to the last row in frame
    intervals (negative: bottom row first); mode "gyro" (rotation over the row time from the sensors' omega, the rest of the flow
    held constant) or "flow" (constant image velocity, no sensor needed); anchor = the row fraction the frame's time stamp belongs
    to; rows None = the frame height of the run; omega_gain turns the sensors' omega into radians per frame interval."""
    readout: float
    mode: str = "gyro"
    anchor: float = 0.5
    rows: int = None
    omega_gain: float = 1.0

    def setting(self):
        """The ofk.RShutter structure (range-checked)."""
        return ofk.rshutter_setting(self.mode, self.readout, self.anchor, self.rows, self.omega_gain)


@dataclass
class PipelineConfig:
    max_corners: int = 500
    quality: float = 0.01
    min_distance: float = 10.0
    block_size: int = 7
    win: int = 15
    max_level: int = 3
    max_count: int = 20
    eps: float = 0.03
    min_eig_thr: float = 1e-4
    solve_variant: int = ofk.SOLVE_NODE
    use_feasibility: bool = False
    feas_T: float = 0.0
    # LK start positions from the sensor model (ofk.h: ofk_set_lk_seed): "off", "model" (omega and the prior velocity) or
    # "rotation" (omega alone); seed_gain scales the predicted flow (omega per second against flow per frame)
    lk_seed: str = "off"
    seed_gain: float = 1.0
    # robust velocity solve (ofk.h: ofk_set_robust): "off", "huber" or "tukey"; robust_c None = 1.345 / 4.685; a sampled start of
    # robust_hypotheses two-point solves, robust_iters reweighting rounds; robust_drop: stream steps drop zero-weight points
    robust: str = "off"
    robust_c: float = None
    robust_iters: int = 5
    robust_hypotheses: int = 64
    robust_seed: int = 0
    robust_drop: bool = False
    # track gates behind LK (ofk.h: ofk_set_track_gate): fb_check "off", "plain" (track the result back from where it landed) or
    # "seeded" (the backward search starts at the original point); a point stays tracked when it comes home within fb_thr pixels;
    # fb_level: pyramid depth of the backward pass, -1 = max_level; err_max > 0 also drops points whose LK err exceeds it
    fb_check: str = "off"
    fb_thr: float = 0.5
    fb_level: int = -1
    err_max: float = 0.0
    # lighting-insensitive LK (ofk.h: ofk_set_lk_light): None, "bias" (a brightness offset per window), "gain" (a gain and an offset)
    # or an ofk.LkLight; the forward LK and the backward pass of fb_check then track under it
    lk_light: object = None
    # corner grid (ofk.h: ofk_set_corner_grid): at most grid_cap corners per grid_cell x grid_cell pixel cell in every selection,
    # grid_cell 0 = off; grid_max_rank > 0: only that many leading candidates are looked at
    grid_cell: int = 0
    grid_cap: int = 0
    grid_max_rank: int = 0
    # velocity covariance (ofk.h: ofk_set_cov): "off", "propagate" (first-order propagation of the six input sigmas through the solve)
    # or "residual" (flow and position terms from the solve's own residual); sigma_flow_px / sigma_pos_px in pixels, sigma_omega a
    # scalar or three values, omega_from_imu: the resident IMU state's angular-velocity variances; cov_filter: the filter's correct
    # uses the covariance (+ r_floor I) in the place of its constant R; nis_max > 0 skips a correct whose NIS exceeds it
    cov: str = "off"
    sigma_flow_px: float = 0.0
    sigma_pos_px: float = 0.0
    sigma_d: float = 0.0
    sigma_omega: object = 0.0
    sigma_normal: float = 0.0
    sigma_offset: float = 0.0
    omega_from_imu: bool = False
    cov_filter: bool = False
    r_floor: float = 0.0
    nis_max: float = 0.0
    # joint velocity and rotation solve (ofk.h: ofk_set_joint): the gyro refined from the flow behind every solve; joint_sigma_flow_px
    # the flow noise in pixels; omega_prior None (every axis free), a scalar or three values (rad per frame; inf: free, 0: held);
    # omega_prior_from_imu: the resident IMU state's angular-velocity variances under use_imu
    joint: bool = False
    joint_sigma_flow_px: float = 0.2
    omega_prior: object = None
    omega_prior_from_imu: bool = False
    # plane solve (ofk.h: ofk_set_plane): the ground normal refined from the flow behind every solve; plane_sigma_flow_px the flow noise
    # in pixels; normal_prior None (the tilt is free) or its standard deviation in radians (0: held); plane_sigma_max the largest
    # predicted 1 sigma of the normal's angle that is accepted; range_beam the range sensor's direction in the camera frame
    plane: bool = False
    plane_sigma_flow_px: float = 0.2
    normal_prior: object = None
    plane_sigma_max: float = 0.1
    range_beam: tuple = (0.0, 0.0, 1.0)
    plane_iters: int = 6
    # epipolar solve (ofk.h: ofk_set_epipolar): velocity and per-point inverse depths over ground that is no plane, behind every solve;
    # epi_anchor_px the radius in pixels around the foot of range_beam inside which the ground is the sensors' plane (inf: every kept
    # point); epi_anchor_min the fewest anchor points; epi_sigma_max the largest predicted 1 sigma of the direction that is accepted
    # (radians); epi_weights "one" (the robust weights are ignored) or "robust"
    epipolar: bool = False
    epi_anchor_px: float = float("inf")
    epi_anchor_min: int = 5
    epi_sigma_max: float = ofk.EPI_SIGMA_MAX
    epi_weights: str = "one"
    # exclusion zones (ofk.h: ofk_set_zones; streams only): None or "hull"; rejects of the solve stage closer than zone_link pixels
    # per axis form a cluster, one of at least zone_min becomes a zone (its hull grown by zone_radius) that moves with the cluster's
    # mean flow, keeps the re-detection out and lives zone_ttl steps behind its last refresh; at most zone_max zones per stream
    zones: str = None
    zone_link: int = 48
    zone_min: int = 3
    zone_radius: int = 20
    zone_ttl: int = 30
    zone_max: int = 16
    # camera model (ofk.h: ofk_set_camera): None, or a CameraModel whose lens distortion is undone on the device in front of the solve
    # stage; the sensors' scaling, cx, cy are then camera.sensor_slots()
    camera: object = None
    # rolling shutter (ofk.h: ofk_set_rolling_shutter): None, or a RollingShutter whose per-row capture time is undone on the device
    # in front of the solve stage
    rolling_shutter: object = None
    # finite motion (ofk.h: ofk_set_finite_motion): None, True (the defaults) or an ofk.FiniteMotion: the frame pair's exact rotation
    # and plane displacement are written into the points on the device in front of the solve stage; the velocity is then the
    # displacement per frame interval
    finite_motion: object = None
    # gyro bias (ofk.h: ofk_set_gyro_bias): None, True (the defaults) or an ofk.GyroBias: every stream filters its gyro's bias from the
    # flow and takes it out of omega in front of each step; FlowPipeline ignores it (independent pairs carry no state)
    gyro_bias: object = None
    # track table (ofk.h: ofk_set_track_table): None, True (the table alone) or an ofk.TrackTable: every stream keeps an id, an age, a
    # birth and the last flow per track on the device, and with seed "flow" starts LK at each track's position plus that flow;
    # FlowPipeline ignores it (independent pairs have no tracks)
    track_table: object = None
    # depth per track (ofk.h: ofk_set_track_depth): None, True (the defaults) or an ofk.TrackDepth: every stream filters an inverse
    # depth per row of its track table (which must be on) and solves a velocity from the depths of the earlier frames;
    # FlowPipeline ignores it
    track_depth: object = None
    # track templates (ofk.h: ofk_set_track_template): None, True (the defaults) or an ofk.TrackTemplate: every stream keeps the patch
    # each track of its table (which must be on) was born with, scores the tracked window against it through the accumulated image
    # deformation, drops the rows that no longer match and pulls the others back onto it; FlowPipeline ignores it
    track_template: object = None
    # keyframe (ofk.h: ofk_set_keyframe): None, True (the defaults) or an ofk.Keyframe: every stream solves its displacement against a
    # held frame of its track table (which must be on) and reports a position that does not drift with the flow; FlowPipeline
    # ignores it
    keyframe: object = None
    # keyframe_rotation (ofk.h: ofk_set_keyframe_rotation): None, True (the defaults) or an ofk.KeyframeRotation: the keyframe's solve
    # refines the accumulated rotation together with the translation; it needs keyframe on
    keyframe_rotation: object = None
    # keyframe_map (ofk.h: ofk_set_keyframe_map): None, True (the defaults) or an ofk.KeyframeMap: the keyframe's translation is
    # solved against the per-track depths frozen at the keyframe, not the ground plane; it needs keyframe and track_depth on;
    # FlowPipeline ignores it
    keyframe_map: object = None
    # pos_filter (ofk.h: ofk_set_pos_filter): None, True (the defaults) or an ofk.PosFilter: every stream fuses the keyframe's
    # displacement, the step's velocity and position fixes in a filter with a cloned state; it needs keyframe on; FlowPipeline ignores it
    pos_filter: object = None
    # stabilise (ofk.h: ofk_set_stabilise): None, True (the defaults) or an ofk.Stabilise: every stream step leaves the step's new gray
    # frame warped into the view of the stream's keyframe on the device; it needs keyframe on and no rolling shutter, and beside a
    # camera model it needs rectify on; FlowPipeline ignores it
    stabilise: object = None
    # rectify (ofk.h: ofk_set_rectify): None, True (the defaults) or an ofk.Rectify: with a camera model on, the stabilised view is
    # accepted and every step's raw frame is warped through the lens's forward map into the ideal view; inert without a camera or
    # without stabilise; FlowPipeline ignores it
    rectify: object = None

    # the three parameter sets the reference carries inline
    @classmethod
    def node(cls):               # velocity_measurment_node:96-107
        return cls(max_corners=100, quality=0.7, min_distance=10, block_size=12, win=15, max_level=3, max_count=20, eps=0.03)

    @classmethod
    def of_module(cls):          # optical_flow_experiments/of_module.py:12-23, T = 0.9 (:55), the inline [p]x / dist_i system (:136-146)
        return cls(max_corners=50, quality=0.3, min_distance=20, block_size=32, win=15, max_level=3, max_count=10, eps=0.5,
                   solve_variant=ofk.SOLVE_OFMODULE, feas_T=0.9)

    @classmethod
    def evaluate_exp(cls):       # flight_experiments/evaluate_exp.py:37-48
        return cls(max_corners=20, quality=0.7, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)

    @classmethod
    def baseline_1080p(cls):     # BASELINE.json configs[1]: 500 corners, 3-level pyramid
        return cls(max_corners=500, quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)

    def robust_setting(self):
        """The ofk.Robust structure of this configuration, None when the robust solve is off."""
        if self.robust == "off":
            return None
        return ofk.robust_setting(self.robust, self.robust_c, self.robust_iters, self.robust_hypotheses, self.robust_seed, self.robust_drop)

    def track_gate_setting(self):
        """The ofk.TrackGate structure of this configuration, None when both gates are off."""
        if self.fb_check == "off" and self.err_max == 0.0:
            return None
        return ofk.track_gate_setting(self.fb_check, self.fb_thr, self.fb_level, self.err_max)

    def lk_light_setting(self):
        """The ofk.LkLight structure of this configuration, None when the lighting-insensitive LK is off."""
        return ofk._light(self.lk_light)

    def corner_grid_setting(self):
        """The ofk.CornerGrid structure of this configuration, None when the grid is off."""
        if self.grid_cell == 0:
            return None
        return ofk.corner_grid_setting(self.grid_cell, self.grid_cap, self.grid_max_rank)

    def cov_setting(self):
        """The ofk.Cov structure of this configuration, None when the covariance is off."""
        if self.cov == "off":
            return None
        return ofk.cov_setting(self.cov, self.sigma_flow_px, self.sigma_pos_px, self.sigma_d, self.sigma_omega, self.sigma_normal,
                               self.sigma_offset, self.omega_from_imu, self.cov_filter, self.r_floor, self.nis_max)

    def joint_setting(self):
        """The ofk.Joint structure of this configuration, None when the joint solve is off."""
        if not self.joint:
            return None
        return ofk.joint_setting(True, self.joint_sigma_flow_px, self.omega_prior, self.omega_prior_from_imu)

    def plane_setting(self):
        """The ofk.Plane structure of this configuration, None when the plane solve is off."""
        if not self.plane:
            return None
        return ofk.plane_setting(True, self.plane_sigma_flow_px, self.normal_prior, self.plane_sigma_max, self.range_beam, self.plane_iters)

    def epipolar_setting(self):
        """The ofk.Epipolar structure of this configuration, None when the epipolar solve is off."""
        if not self.epipolar:
            return None
        return ofk.epipolar_setting(True, self.epi_anchor_px, self.epi_anchor_min, self.epi_sigma_max, self.range_beam, self.epi_weights)

    def zones_setting(self):
        """The ofk.Zones structure of this configuration, None when the zones are off."""
        if self.zones is None or self.zones == "off":
            return None
        return ofk.zones_setting(self.zones, self.zone_link, self.zone_min, self.zone_radius, self.zone_ttl, self.zone_max)

    def camera_setting(self):
        """The ofk.Camera structure of this configuration, None when no camera model is set."""
        if self.camera is None:
            return None
        m = self.camera.setting() if hasattr(self.camera, "setting") else self.camera
        return None if m.model == ofk.CAMERA_OFF else m

    def rolling_shutter_setting(self):
        """The ofk.RShutter structure of this configuration, None when no rolling shutter is set."""
        if self.rolling_shutter is None:
            return None
        m = self.rolling_shutter.setting() if hasattr(self.rolling_shutter, "setting") else self.rolling_shutter
        return None if m.mode == ofk.RS_OFF else m

    def _struct_setting(self, name, cls, maker, rebuild=True):
        """The setting `name` of this configuration: None / False (off), True (the maker's defaults) or an ofk structure of `cls`
        -> the structure, None when it is off.  rebuild: made again by `maker` from its fields, by keyword: range-checked."""
        m = getattr(self, name)
        if m is None or m is False:
            return None
        m = maker() if m is True else m
        if not isinstance(m, cls):
            raise ValueError(f"{name} {m!r} is neither None, True nor an ofk.{cls.__name__}")
        if rebuild:
            m = maker(**{f: tuple(v) if hasattr(v, "__len__") else v for f, v in ((f[0], getattr(m, f[0])) for f in cls._fields_)})
        return None if m.mode == 0 else m                        # every one's OFF is 0

    def finite_motion_setting(self):
        """The ofk.FiniteMotion structure of this configuration, None when the finite motion is off."""
        return self._struct_setting("finite_motion", ofk.FiniteMotion, ofk.finite_motion_setting)

    def gyro_bias_setting(self):
        """The ofk.GyroBias structure of this configuration, None when the gyro bias is off."""
        return self._struct_setting("gyro_bias", ofk.GyroBias, ofk.gyro_bias_setting, rebuild=False)

    def track_table_setting(self):
        """The ofk.TrackTable structure of this configuration, None when the track table is off."""
        return self._struct_setting("track_table", ofk.TrackTable, ofk.track_table_setting)

    def track_depth_setting(self):
        """The ofk.TrackDepth structure of this configuration, None when the depths are off."""
        return self._struct_setting("track_depth", ofk.TrackDepth, ofk.track_depth_setting)

    def keyframe_setting(self):
        """The ofk.Keyframe structure of this configuration, None when the keyframe is off."""
        return self._struct_setting("keyframe", ofk.Keyframe, ofk.keyframe_setting)

    def keyframe_rotation_setting(self):
        """The ofk.KeyframeRotation structure of this configuration, None when the rotation is not refined."""
        m = self._struct_setting("keyframe_rotation", ofk.KeyframeRotation, ofk.keyframe_rotation_setting)
        if m is not None and self.keyframe_setting() is None:
            raise ValueError("keyframe_rotation needs keyframe on")
        return m

    def keyframe_map_setting(self):
        """The ofk.KeyframeMap structure of this configuration, None when the key solve is the plane's."""
        m = self._struct_setting("keyframe_map", ofk.KeyframeMap, ofk.keyframe_map_setting)
        if m is not None and (self.keyframe_setting() is None or self.track_depth_setting() is None):
            raise ValueError("keyframe_map needs keyframe and track_depth on")
        if m is not None and self.keyframe_rotation_setting() is not None:
            raise ValueError("keyframe_map beside keyframe_rotation: the joint solve over map rows is not built")
        return m

    def pos_filter_setting(self):
        """The ofk.PosFilter structure of this configuration, None when the position filter is off."""
        if self.pos_filter is None or self.pos_filter is False:
            return None
        m = ofk.pos_filter_setting() if self.pos_filter is True else self.pos_filter
        if not isinstance(m, ofk.PosFilter):
            raise ValueError(f"pos_filter {m!r} is neither None, True nor an ofk.PosFilter")
        m = ofk.pos_filter_setting(*[getattr(m, n) for n, _ in ofk.PosFilter._fields_])   # range-checked
        if m.mode != ofk.POSF_OFF and self.keyframe_setting() is None:
            raise ValueError("pos_filter needs keyframe on")
        return None if m.mode == ofk.POSF_OFF else m

    def stabilise_setting(self):
        """The ofk.Stabilise structure of this configuration, None when no stabilised view is kept."""
        m = self._struct_setting("stabilise", ofk.Stabilise, ofk.stabilise_setting)
        if m is not None and self.keyframe_setting() is None:
            raise ValueError("stabilise needs keyframe on")
        if m is not None and self.rolling_shutter_setting() is not None:
            raise ValueError("stabilise beside a rolling shutter: the homography holds between global-shutter images, and nothing undoes the row time in the frame")
        if m is not None and self.camera_setting() is not None and self.rectify_setting() is None:
            raise ValueError("stabilise beside a camera model without rectify: a raw frame needs the lens's map behind the warp (rectify=True)")
        return m

    def rectify_setting(self):
        """The ofk.Rectify structure of this configuration, None when the view is not resampled through the lens."""
        return self._struct_setting("rectify", ofk.Rectify, ofk.rectify_setting)

    def track_template_setting(self):
        """The ofk.TrackTemplate structure of this configuration, None when the templates are off."""
        return self._struct_setting("track_template", ofk.TrackTemplate, ofk.track_template_setting)

    def to_params(self):
        return ofk.Params(int(self.max_corners), float(self.quality), float(self.min_distance), int(self.block_size),
                          int(self.win), int(self.max_level), int(self.max_count), float(self.eps), float(self.min_eig_thr),
                          int(self.solve_variant), 1 if self.use_feasibility else 0, float(self.feas_T))


@dataclass
class FilterModel:
    """Matrices of the per-stream linear Kalman filter (k_kf; ofk_kf_predict_update / the resident filter of FlowStream).

    kf3()  the reference's filter, of_module.py:63-76: cv2.KalmanFilter(3, 3, 0) with F = B = H = I, Q = 1e-5 I, R = 10 I,
           P0 = 0.1 I, x0 = 0; predict(control) every frame (:122), correct(-v_obs) (:152).
    ekf6() the build-defined 6-state superset BASELINE.json configs[2] asks for (the reference has no such filter and no GPS
           data: DESIGN.md §2a): x = [v, b] with b the accelerometer bias in the velocity frame,
               v' = v + u - b dt,   b' = b          F = [[I, -dt I], [0, I]],  B = [[I], [0]]
           where the control u is the dead-reckoning increment R (a - 9.81 n) dt of node:80-82; the optical fix measures v
           (H = [I 0], z = -v_obs as in the reference); with gps=True a second velocity measurement (what a GPS receiver's
           velocity output would deliver) is stacked under it: H = [[I 0], [I 0]], R = diag(r I, r_gps I).  Both models are
           linear, so the "EKF" is the Kalman filter itself; kf3 is its restriction to the first three states, and with
           dt = 0 and no bias noise the v-block of ekf6 reproduces kf3 bit for bit (tested).
    """
    F: np.ndarray
    B: np.ndarray
    H: np.ndarray
    Q: np.ndarray
    R: np.ndarray
    P0: np.ndarray
    x0: np.ndarray

    @property
    def ns(self):
        return self.F.shape[0]

    @property
    def nm(self):
        return self.H.shape[0]

    @property
    def nc(self):
        return self.B.shape[1]

    @classmethod
    def kf3(cls):
        I = np.eye(3)
        return cls(F=I.copy(), B=I.copy(), H=I.copy(), Q=1e-5 * I, R=10.0 * I, P0=0.1 * I, x0=np.zeros(3))

    @classmethod
    def ekf6(cls, dt=1.0 / 30.0, q_v=1e-5, q_b=1e-7, r=10.0, p0=0.1, gps=False, r_gps=1.0):
        I, Z = np.eye(3), np.zeros((3, 3))
        F = np.block([[I, -dt * I], [Z, I]])
        Bm = np.vstack([I, Z])
        H = np.hstack([I, Z])
        R = r * I
        if gps:
            H = np.vstack([H, np.hstack([I, Z])])
            R = np.block([[r * I, Z], [Z, r_gps * I]])
        return cls(F=F, B=Bm, H=H, Q=np.diag([q_v] * 3 + [q_b] * 3), R=R, P0=p0 * np.eye(6), x0=np.zeros(6))


@dataclass
class FusionConfig:
    """What FlowStream.step_fused does between LK and the next frame (ofk_fusion, include/ofk.h)."""
    use_imu: bool = False
    flow: int = ofk.FLOW_LK
    keep: int = ofk.KEEP_STATUS
    filter: bool = False
    control: int = ofk.CONTROL_SENSORS
    z_sign: float = 1.0
    z_source: int = 0
    vel_overwrite: bool = False
    redetect_replace: bool = False
    min_solve: int = 2
    hold_on_skip: bool = False
    model: "FilterModel" = None

    @classmethod
    def of_module(cls, synthetic_flow=True, hold_on_skip=False):
        """The loop of optical_flow_experiments/of_module.py:78-167: kalman.predict(control) -> legacy r_tilde with the predicted
        velocity, keep r - (status - 1) >= T with cv2's uint8 status (a lost point's status-1 wraps to 255: dropped) -> A_i = [p]x / dist_i system -> kalman.correct(-v_obs); tracks := kept points;
        <= 10 tracks: replace by fresh corners.  synthetic_flow reproduces :113-114 (the measured flow overwritten by the
        rotational field of a random omega); False keeps the LK flow the script's TODO asks for.
        Use with PipelineConfig.of_module() (feas_T = 0.9, solve_variant = OFMODULE) and sensors cx, cy = of.pix_trans((480, 640)),
        scaling = 1 (the script works in pixels, :96-102).  hold_on_skip=True (a FlowStream of ONE stream, which is what the script is)
        also reproduces its `continue` at :138: a frame with <= 3 feasible points leaves old_gray and old_pos untouched, so the next
        frame is tracked from the old one; in a batch of streams the frame always advances (one frame swap for all)."""
        return cls(flow=ofk.FLOW_ROTATIONAL if synthetic_flow else ofk.FLOW_LK, keep=ofk.KEEP_LEGACY, filter=True, control=ofk.CONTROL_SENSORS,
                   z_sign=-1.0, z_source=0, redetect_replace=True, min_solve=3, hold_on_skip=bool(hold_on_skip), model=FilterModel.kf3())

    @classmethod
    def node(cls):
        """velocity_measurment_node: IMU dead-reckoning between optical fixes (node:61-89), r_tilde filter with the dead-reckoned
        velocity (:238-245), solve (:257), self.vel = v_uav (:261).  No Kalman filter (the reference node has none)."""
        return cls(use_imu=True, keep=ofk.KEEP_STATUS, filter=False, vel_overwrite=True, min_solve=2)

    @classmethod
    def ekf6(cls, dt=1.0 / 30.0, gps=False, **kw):
        """BASELINE configs[2]/[3]'s "6-state EKF": the node's loop with the build-defined filter FilterModel.ekf6 in place of the
        hard overwrite: predict with the IMU's velocity increments since the last frame, correct with +v_uav (world frame)."""
        return cls(use_imu=True, keep=ofk.KEEP_STATUS, filter=True, control=ofk.CONTROL_IMU, z_sign=1.0, z_source=1, vel_overwrite=False,
                   min_solve=2, model=FilterModel.ekf6(dt=dt, gps=gps, **kw))

    def to_struct(self):
        return ofk.Fusion(1 if self.use_imu else 0, int(self.flow), int(self.keep), 1 if self.filter else 0, int(self.control), float(self.z_sign),
                          int(self.z_source), 1 if self.vel_overwrite else 0, 1 if self.redetect_replace else 0, int(self.min_solve), 1 if self.hold_on_skip else 0)


def _apply_settings(ctx, cfg, zones):
    """The settings a PipelineConfig switches on, on a fresh context, in the order the library's checks were written for; zones:
    whether the exclusion zones, the gyro bias, the track table, the depths per track, the track templates and the keyframe are among
    them (they belong to the stream steps)."""
    if cfg.lk_seed != "off":
        ctx.set_lk_seed(cfg.lk_seed, cfg.seed_gain)
    steps = [(ctx.set_robust, cfg.robust_setting), (ctx.set_track_gate, cfg.track_gate_setting), (ctx.set_lk_light, cfg.lk_light_setting),
             (ctx.set_corner_grid, cfg.corner_grid_setting),
             (ctx.set_cov, cfg.cov_setting), (ctx.set_joint, cfg.joint_setting), (ctx.set_plane, cfg.plane_setting),
             (ctx.set_epipolar, cfg.epipolar_setting)]
    if zones:
        steps += [(ctx.set_zones, cfg.zones_setting), (ctx.set_gyro_bias, cfg.gyro_bias_setting), (ctx.set_track_table, cfg.track_table_setting),
                  (ctx.set_track_depth, cfg.track_depth_setting), (ctx.set_track_template, cfg.track_template_setting),
                  (ctx.set_keyframe, cfg.keyframe_setting), (ctx.set_keyframe_rotation, cfg.keyframe_rotation_setting),
                  (ctx.set_keyframe_map, cfg.keyframe_map_setting), (ctx.set_pos_filter, cfg.pos_filter_setting),
                  (ctx.set_rectify, cfg.rectify_setting), (ctx.set_stabilise, cfg.stabilise_setting)]
    steps += [(ctx.set_camera, cfg.camera_setting), (ctx.set_rolling_shutter, cfg.rolling_shutter_setting),
              (ctx.set_finite_motion, cfg.finite_motion_setting)]
    for setter, setting in steps:                                # every *_setting() is None when its setting is off
        value = setting()
        if value is not None:
            setter(value)


def _ideal_points(ctx, batch):
    """The download of the last point correction that is on: each one's output is the next one's input."""
    if ctx.get_finite_motion().mode != ofk.FM_OFF:
        return ctx.finite_download(batch)
    return ctx.rs_download(batch) if ctx.get_rolling_shutter().mode != ofk.RS_OFF else ctx.camera_download(batch)


class FlowStream:
    """`batch` independent video streams with persistent tracks on the device: the loop of velocity_measurment_node:92-177
    (commented-out blocks restored) / of_module.py:78-167 / evaluate_exp.py:77-121, one frame per `step`.

        fs = FlowStream(1280, 960, batch=1, cfg=PipelineConfig.node(), min_features=20, mask_radius=30)
        tracks, counts = fs.begin(first_frames)                 # goodFeaturesToTrack on the first frames
        records, tracks, counts = fs.step(frames, sensors)      # LK, velocity, status filter, re-detection, frame swap
    """

    def __init__(self, width, height, batch=1, cfg=None, device=0, min_features=20, mask_radius=30, fusion=None):
        self.cfg = cfg or PipelineConfig.node()
        self.batch = batch
        self.min_features, self.mask_radius = int(min_features), int(mask_radius)
        self.ctx = ofk.Context(device, width, height, batch, max(1, self.cfg.max_corners), max(0, self.cfg.max_level))
        self._params = self.cfg.to_params()
        _apply_settings(self.ctx, self.cfg, zones=True)
        self.fusion = fusion
        if fusion is not None:                                  # the per-stream filter state lives on the device from here on
            self._fusion = fusion.to_struct()
            self.ctx.imu_reset(batch)
            if fusion.filter:
                self.ctx.filter_configure(fusion.model or FilterModel.kf3(), batch)

    def push_imu(self, msgs, counts=None):
        """The IMU messages received since the last frame ([B, M, 15], layout ofk.h OFK_IMU_MSG), applied to the resident state."""
        self.ctx.imu_push(msgs, counts)

    def step_fused(self, next_frames, sensors):
        """One frame with the filters in the loop (ofk_stream_step_fused): BGR frames [B,h,w,3] or a list of B JPEG streams.
        Returns (records, fused [B,8] = filter state x[0..5], trace P, solved, tracks, counts)."""
        if self.fusion is None:
            raise ValueError("construct FlowStream(..., fusion=FusionConfig...) for step_fused")
        return self.ctx.stream_step_fused(next_frames, sensors, self._params, self._fusion, self.min_features, self.mask_radius)

    def track_gate_stats(self):
        """[batch, 4] int32 of the latest step with a track gate on: forward-tracked points, of those lost by the backward pass, of
        the rest beyond fb_thr, of the rest over err_max."""
        return self.ctx.track_gate_stats(self.batch)

    def corner_grid_stats(self):
        """[batch, 2] int32 of the latest detection (begin or re-detection) with a corner grid on: corners accepted, candidates examined."""
        return self.ctx.corner_grid_stats(self.batch)

    def planes(self):
        """[batch, 32] plane records (ofk.h: ofk_set_plane) of the latest step with the plane solve on: rec[:, 0:3] is the refined normal,
        rec[:, 3] the refined distance, rec[:, 4:6] the tilt, rec[:, 10] the flag, rec[:, 14] the predicted 1 sigma of the normal's angle,
        ofk.cov_matrix(rec[:, 20:26]) C_v."""
        return self.ctx.plane_download(self.batch)

    def structure(self):
        """The epipolar record [batch, 32] and point rows [batch, max_pts, 4] (ofk.h: ofk_set_epipolar) of the latest step with the
        epipolar solve on: rec[:, 0:3] is the direction t^, rec[:, 3] the scale s, rec[:, 4] the flow noise estimated from the
        constraint, rec[:, 10] the flag, rec[:, 17] the predicted 1 sigma of the direction, ofk.cov_matrix(rec[:, 25:31]) C_v;
        pts[..., 0] the inverse depths rho_i, pts[..., 1] the flow across the epipolar line, pts[..., 3] the point flag."""
        return self.ctx.epipolar_download(self.batch)

    def rotations(self):
        """[batch, 32] joint records (ofk.h: ofk_set_joint) of the latest step with the joint solve on: rec[:, 0:3] is the refined omega,
        rec[:, 3:6] its correction, rec[:, 10] the flag, ofk.cov_matrix(rec[:, 15:21]) C_omega, ofk.cov_matrix(rec[:, 21:27]) C_v."""
        return self.ctx.joint_download(self.batch)

    def gyro_bias(self):
        """[batch, 32] bias records (ofk.h: ofk_set_gyro_bias) of the latest step with the gyro bias on: rec[:, 0:3] is the bias,
        ofk.cov_matrix(rec[:, 3:9]) its covariance, rec[:, 9:12] the raw omega, rec[:, 12:15] the omega the step used, rec[:, 18] the flag."""
        return self.ctx.gyro_bias_download(self.batch)

    def covariances(self):
        """[batch, 24] cov records (ofk.h: ofk_set_cov) of the latest step with the covariance on; ofk.cov_matrix(rec[:, 0:6]) is C_v,
        rec[:, 6:12] C_uav, 14 the NIS of the filter's correct, 15 whether it was gated."""
        return self.ctx.cov_download(self.batch)

    def zones(self):
        """The streams' exclusion zones behind the latest step (ofk.Context.zones_download): dict(zones [batch,16,67] i32, motion
        [batch,16,4] f32, stats [batch,8] i32)."""
        return self.ctx.zones_download(self.batch)

    def ideal_points(self):
        """(prev, next) [batch, max_pts, 2] f32: the points the solve stage of the latest step saw (camera model, rolling shutter or
        finite motion on)."""
        return _ideal_points(self.ctx, self.batch)

    def track_table(self):
        """The streams' track tables behind the latest begin or step (ofk.h: ofk_set_track_table): dict(ids, age, birth_step, birth_xy,
        flow_xy: per stream the rows of the tracks that call returned, in their order; step_ids: per stream the ids of the rows the
        latest step tracked, stream_last_points' rows; stats [batch, 8] i32: count, kept, lost, born, oldest age, step, next_id, rows
        seeded from their flow)."""
        t = self.ctx.track_table_download(self.batch)
        st = t["stats"]
        out = {k: [t[k][b, :st[b, 0]] for b in range(self.batch)] for k in ("ids", "age", "birth_step", "birth_xy", "flow_xy")}
        out["step_ids"] = [t["step_ids"][b, :st[b, 1] + st[b, 2]] for b in range(self.batch)]
        out["stats"] = st
        return out

    def _track_rows(self, d, keys):
        """Per stream the rows of download d[k], k in keys, of the tracks that the latest step returned, in their order, and under
        "ids" their ids from the track table."""
        t = self.ctx.track_table_download(self.batch)
        cnt = t["stats"][:, 0]
        out = {k: [d[k][b, :cnt[b]] for b in range(self.batch)] for k in keys}
        out["ids"] = [t["ids"][b, :cnt[b]] for b in range(self.batch)]
        return out

    def depths(self):
        """The streams' depths per track behind the latest step (ofk.h: ofk_set_track_depth): dict(rho, var, nobs, ids: per stream the
        rows of the tracks that step returned, in their order, ids joined from the track table; rec [batch, 32]: rec[:, 0:3] is v_map,
        rec[:, 3] its flag, rec[:, 4] the mature rows it used, ofk.cov_matrix(rec[:, 10:16]) C_map)."""
        d = self.ctx.track_depth_download(self.batch)
        return dict(self._track_rows(d, ("rho", "var", "nobs")), rec=d["rec"])

    def templates(self):
        """The streams' track templates behind the latest step (ofk.h: ofk_set_track_template): dict(tmpl, A, ncc, flag, tstate, ids: per
        stream the rows of the tracks that step returned, in their order, ids joined from the track table; tmpl as
        [rows, win + 2, win + 2]; rec [batch, 32]: rec[:, 0:4] the step map M, rec[:, 4:6] t, rec[:, 6] the fit flag, rec[:, 10:20] the
        counts and the largest move)."""
        d = self.ctx.track_template_download(self.batch)
        e = self.ctx.get_track_template().win + 2
        out = dict(self._track_rows(d, ("A", "ncc", "flag", "tstate", "tmpl")), rec=d["rec"])
        out["tmpl"] = [m[:, :e * e].reshape(-1, e, e) for m in out["tmpl"]]
        return out

    def position(self):
        """The streams' position against their keyframes behind the latest step (ofk.h: ofk_set_keyframe): dict(pos, D, T [batch, 3]:
        the position, the displacement since the keyframe and the key solve's translation; flag [batch] (ofk.KEY_SOLVED, _UNSOLVED,
        _NONE); with ofk_set_keyframe_rotation on T, pos and C_T are those of the solve that stands; C_T [batch, 3, 3]; R_acc [batch, 3, 3]; live, members_at_key, key_step, keyframes, dead_reckoned, reason [batch];
        ids: per stream the ids of the keyframe's members among the tracks that step returned, from the track table; rec)."""
        d = self.ctx.keyframe_download(self.batch)
        rows, rec = self._track_rows(d, ("member",)), d["rec"]
        out = dict(pos=rec[:, 13:16].copy(), D=rec[:, 10:13].copy(), T=rec[:, 0:3].copy(), flag=rec[:, 3].astype(np.int32),
                   C_T=ofk.cov_matrix(rec[:, 20:26]), R_acc=d["R_acc"], rec=rec)
        for k, s in (("members_at_key", 7), ("key_step", 8), ("reason", 9), ("keyframes", 26), ("dead_reckoned", 27), ("live", 28)):
            out[k] = rec[:, s].astype(np.int32)
        out["ids"] = [i[m != 0] for i, m in zip(rows["ids"], rows["member"])]
        return out

    def key_rotation(self):
        """The keyframes' rotation refined from the flow behind the latest step (ofk.h: ofk_set_keyframe_rotation): dict(delta
        [batch, 3]; R_hat, C_delta [batch, 3, 3]; flag [batch] (ofk.KEYROT_*); prior [batch, 3]: the prior's sigma per axis (0: held);
        eig [batch, 3]: the reduced system's eigenvalues; iterations [batch]; rec [batch, 40])."""
        rec = self.ctx.keyframe_rotation_download(self.batch)
        return dict(delta=rec[:, 0:3].copy(), R_hat=rec[:, 4:13].reshape(-1, 3, 3).copy(), C_delta=ofk.cov_matrix(rec[:, 13:19]),
                    flag=rec[:, 3].astype(np.int32), prior=rec[:, 28:31].copy(), eig=rec[:, 25:28].copy(), iterations=rec[:, 31].astype(np.int32),
                    rec=rec)

    def key_map(self):
        """The keyframes' maps behind the latest step (ofk.h: ofk_set_keyframe_map): dict(flag [batch] (ofk.KEYMAP_*); map_rows,
        live_rows, rows, rows_gated, captured, captured_for [batch]; weight_sum, spread [batch]; T_plain [batch, 3]: the plain first
        solve's translation where both ran; key_rho, key_var, ids: per stream the rows of the tracks that step returned, in their
        order, ids joined from the track table; rec [batch, 32])."""
        d = self.ctx.keyframe_map_download(self.batch)
        rec = d["rec"]
        out = dict(self._track_rows(d, ("key_rho", "key_var")), flag=rec[:, 0].astype(np.int32), weight_sum=rec[:, 5].copy(), spread=rec[:, 6].copy(),
                   T_plain=rec[:, 7:10].copy(), rec=rec)
        for k, s in (("map_rows", 1), ("live_rows", 2), ("rows", 3), ("rows_gated", 4), ("captured", 10), ("captured_for", 11)):
            out[k] = rec[:, s].astype(np.int32)
        return out

    def stabilised(self, frames=True):
        """The stabilised view behind the latest step (ofk.h: ofk_set_stabilise): dict(frames [batch, h, w] u8: the step's new gray
        frame in the view of the stream's first keyframe (frames=False: left on the device); M [batch, 3, 3]: view pixel -> frame pixel;
        Bv, R [batch, 3, 3], T [batch, 3]; flag [batch] (ofk.STAB_*); rebase [batch]: the step's re-base reason (0: none); cover
        [batch]: the share of the view the frame filled; covered, steps, rebases, approx, rekeyed [batch]; rec [batch, 48])."""
        h, w = self.ctx.max_h, self.ctx.max_w
        d = self.ctx.stab_download(self.batch, h, w, frames=frames)
        rec = d["rec"]
        out = dict(M=rec[:, 0:9].reshape(-1, 3, 3).copy(), Bv=rec[:, 9:18].reshape(-1, 3, 3).copy(), R=rec[:, 18:27].reshape(-1, 3, 3).copy(),
                   T=rec[:, 27:30].copy(), flag=rec[:, 30].astype(np.int32), rebase=rec[:, 31].astype(np.int32), covered=d["covered"],
                   cover=d["covered"] / float(h * w), rec=rec)
        for k, slot in (("steps", 32), ("rebases", 33), ("approx", 34), ("rekeyed", 35)):
            out[k] = rec[:, slot].astype(np.int32)
        if frames:
            out["frames"] = d["frames"]
        return out

    def position_input(self, du=None, fix=None, fix_sigma=None):
        """What the position filter takes in with the next step that is not held (ofk.h: ofk_pos_filter_input): du [batch, 3] the
        velocity increment over the step in the world frame (None: none); fix [batch, 3] an absolute position with fix_sigma (a
        number, [3] or [batch, 3]; None with a fix: ValueError).  A row of fix with a NaN marks a stream without a fix."""
        row = np.zeros((self.batch, ofk.POSF_INPUT), np.float64)
        if du is not None:
            row[:, 0:3] = np.broadcast_to(np.asarray(du, np.float64), (self.batch, 3))
        if fix is not None:
            if fix_sigma is None:
                raise ValueError("position_input: a fix needs fix_sigma")
            f = np.broadcast_to(np.asarray(fix, np.float64), (self.batch, 3))
            has = np.isfinite(f).all(axis=1)
            row[:, 3] = has
            row[:, 4:7] = np.where(has[:, None], f, 0.0)
            row[:, 7:10] = np.broadcast_to(np.asarray(fix_sigma, np.float64), (self.batch, 3))
        self.ctx.pos_filter_input(row)

    def fused_position(self):
        """The streams' position filter behind the latest step (ofk.h: ofk_set_pos_filter): dict(p, v, b, c [batch, 3]; P [batch, 12,
        12]; P_pp [batch, 3, 3]; nis, outcome [batch, 3] and innovation [batch, 3, 3] of the velocity, displacement and fix updates
        (outcome ofk.POSF_*); cloned [batch]; counts: dict(steps, fresh, clones [batch], velocity, displacement, fix [batch, 3]:
        applied, gated, refused); rec [batch, 48])."""
        d = self.ctx.pos_filter_download(self.batch)
        x, rec, ist = d["x"], d["rec"], d["istate"]
        upd = rec[:, 25:40].reshape(-1, 3, 5)
        return dict(p=x[:, 0:3].copy(), v=x[:, 3:6].copy(), b=x[:, 6:9].copy(), c=x[:, 9:12].copy(), P=d["P"], P_pp=d["P"][:, 0:3, 0:3].copy(),
                    nis=upd[:, :, 1].copy(), outcome=upd[:, :, 0].astype(np.int32), innovation=upd[:, :, 2:5].copy(), cloned=rec[:, 40].astype(np.int32),
                    counts=dict(steps=ist[:, 0].copy(), fresh=ist[:, 1].copy(), clones=ist[:, 2].copy(), velocity=ist[:, 4:7].copy(),
                                displacement=ist[:, 7:10].copy(), fix=ist[:, 10:13].copy()), rec=rec)

    def begin(self, first_bgr):
        return self.ctx.stream_begin(first_bgr, self._params)

    def step(self, next_bgr, sensors):
        return self.ctx.stream_step(next_bgr, sensors, self._params, self.min_features, self.mask_radius)

    def begin_jpeg(self, first_streams):
        """begin() with the frames as the node receives them: one JPEG stream (CompressedImage payload) per camera."""
        return self.ctx.stream_begin_jpeg(first_streams, self._params)

    def step_jpeg(self, next_streams, sensors):
        return self.ctx.stream_step_jpeg(next_streams, sensors, self._params, self.min_features, self.mask_radius)

    def close(self):
        self.ctx.close()


def auto_streams(width, height, batch):
    """Free-running slices of ofk_pairs_run for a frame size (streams=None): ONE stage chain for large frames - the response kernel
    is the longest stage and wave-sized selection / solve workgroups fit beside it - and TWO for frames up to 640 x 480 in batches of
    at least 256 pairs, where LK is the longest stage, the latency-bound phases (selection, solve) weigh more and a second chain fills
    them: 1024 pairs of 640 x 480: 343-359 k pairs/s on one slice, 380-400 k on two; 1080p and 4K: one slice is 3-6 % faster."""
    return 2 if width * height <= 640 * 480 and batch >= 256 else 1


class FlowPipeline:
    def __init__(self, width, height, batch=1, cfg=None, device=0, streams=1):
        self.cfg = cfg or PipelineConfig.baseline_1080p()
        self.batch = batch
        if streams is None:
            streams = auto_streams(width, height, batch)
        self.streams = streams
        self.ctx = ofk.Context(device, width, height, batch, max(1, self.cfg.max_corners), max(0, self.cfg.max_level))
        self._params = self.cfg.to_params()
        _apply_settings(self.ctx, self.cfg, zones=False)         # pairs_run ignores the zones
        if streams > 1:
            self.ctx.set_streams(streams)

    def upload(self, prev_bgr, next_bgr, sensors):
        self.ctx.pairs_upload(prev_bgr, next_bgr)
        self.ctx.pairs_set_sensors(sensors)

    def upload_jpeg(self, prev_streams, next_streams, sensors):
        """The same from baseline JPEG streams (CompressedImage payloads): decoded on the device, 15-20x less PCIe traffic."""
        self.ctx.pairs_upload_jpeg(prev_streams, next_streams)
        self.ctx.pairs_set_sensors(sensors)

    def run_jpeg_batches(self, batches, sensors, on_step=None):
        """The pipeline over an iterable of (prev_streams, next_streams) batches with the ingest double-buffered: a helper thread
        parses, stages and uploads batch k + 1 (ofk_jpeg_stage, slot (k + 1) & 1) while this thread decodes batch k on the device
        (ofk_pairs_upload_staged) and queues its ofk_pairs_run.  `sensors`: one [B, 28] array for all batches or a callable
        k -> array.  on_step(k) is called after step k was queued (e.g. to pick up step k - 1's records).  Returns the number of steps;
        the last one is still running (call sync() / run-download)."""
        from concurrent.futures import ThreadPoolExecutor
        it = iter(batches)
        first = next(it, None)
        if first is None:
            return 0
        n = 0
        with ThreadPoolExecutor(1) as ex:
            fut = ex.submit(self.ctx.jpeg_stage, 0, list(first[0]) + list(first[1]))
            while fut is not None:
                staged = fut.result()
                nxt = next(it, None)
                fut = ex.submit(self.ctx.jpeg_stage, (n + 1) & 1, list(nxt[0]) + list(nxt[1])) if nxt is not None else None
                self.ctx.pairs_upload_staged(n & 1, staged)
                if callable(sensors) or n == 0:
                    self.ctx.pairs_set_sensors(sensors(n) if callable(sensors) else sensors)
                self.run_async()
                if on_step is not None:
                    on_step(n)
                n += 1
        return n

    def track_gate_stats(self):
        """[batch, 4] int32 of the latest run with a track gate on (see FlowStream.track_gate_stats)."""
        return self.ctx.track_gate_stats(self.batch)

    def corner_grid_stats(self):
        """[batch, 2] int32 of the latest run with a corner grid on: corners accepted, candidates examined."""
        return self.ctx.corner_grid_stats(self.batch)

    def planes(self):
        """[batch, 32] plane records (ofk.h: ofk_set_plane) of the latest run with the plane solve on (see FlowStream.planes)."""
        return self.ctx.plane_download(self.batch)

    def structure(self):
        """The epipolar record [batch, 32] and point rows [batch, max_pts, 4] (ofk.h: ofk_set_epipolar) of the latest run with the
        epipolar solve on (see FlowStream.structure)."""
        return self.ctx.epipolar_download(self.batch)

    def rotations(self):
        """[batch, 32] joint records (ofk.h: ofk_set_joint) of the latest run with the joint solve on (see FlowStream.rotations)."""
        return self.ctx.joint_download(self.batch)

    def covariances(self):
        """[batch, 24] cov records (ofk.h: ofk_set_cov) of the latest run with the covariance on (see FlowStream.covariances)."""
        return self.ctx.cov_download(self.batch)

    def ideal_points(self):
        """(prev, next) [batch, max_pts, 2] f32: the points the solve stage of the latest run saw (camera model, rolling shutter or
        finite motion on)."""
        return _ideal_points(self.ctx, self.batch)

    def run_async(self):
        self.ctx.pairs_run(self._params)

    def sync(self):
        self.ctx.sync()

    def run(self, points=True):
        self.run_async()
        return self.ctx.pairs_download(points=points)

    def close(self):
        self.ctx.close()
