"""ofk.py — ctypes binding of libofk.so (include/ofk.h), numpy in / numpy out.

This is the only place the package touches native code.  There is no CPU fallback: if the
shared library is missing or no gfx950 device is usable, importing succeeds (so that
CPU-only tooling can inspect the package) but the first call raises OfkError.
"""
import contextlib
import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libofk.so")

OK, E_INVALID, E_HIP, E_CAPACITY, E_NOGPU = 0, -1, -2, -3, -4
SOLVE_NODE, SOLVE_SIM, SOLVE_OFMODULE = 0, 1, 2
FEAS_RTILDE, FEAS_LEGACY, FEAS_SIM = 0, 1, 2
SENSOR_DOUBLES, RECORD_DOUBLES, SOLVE_DOUBLES = 28, 16, 8
IMU_STATE, IMU_MSG = 24, 15
MAX_DIM = 16384          # ofk_create rejects larger frames
STAGES = ("gray", "pyr", "eig", "nms", "select", "lk", "solve")

# every entry point include/ofk.h declares (tests/test_abi.py checks the library exports them all)
SYMBOLS = (
    "ofk_version", "ofk_last_error", "ofk_device_count", "ofk_create", "ofk_destroy", "ofk_sync", "ofk_device_sync",
    "ofk_gray_bgr8", "ofk_pyr_down_u8", "ofk_pyramid_u8", "ofk_scharr_s16", "ofk_warp_perspective", "ofk_warp_lens", "ofk_mineig_response", "ofk_select_corners",
    "ofk_good_features", "ofk_lk_pyr", "ofk_lk_pyr_ex", "ofk_predict_points", "ofk_set_lk_seed", "ofk_get_lk_seed", "ofk_flow_model", "ofk_feasibility", "ofk_velocity_solve", "ofk_imu_propagate",
    "ofk_set_robust", "ofk_get_robust", "ofk_robust_download", "ofk_velocity_solve_robust", "ofk_robust_pairs",
    "ofk_set_cov", "ofk_get_cov", "ofk_cov_download", "ofk_velocity_solve_cov",
    "ofk_set_joint", "ofk_get_joint", "ofk_joint_download", "ofk_velocity_solve_joint",
    "ofk_set_gyro_bias", "ofk_get_gyro_bias", "ofk_gyro_bias_reset", "ofk_gyro_bias_download", "ofk_gyro_bias_step",
    "ofk_set_plane", "ofk_get_plane", "ofk_plane_download", "ofk_velocity_solve_plane",
    "ofk_set_epipolar", "ofk_get_epipolar", "ofk_epipolar_download", "ofk_epipolar_points_download", "ofk_velocity_solve_epipolar",
    "ofk_set_track_gate", "ofk_get_track_gate", "ofk_track_gate_download", "ofk_lk_pyr_fb",
    "ofk_set_lk_light", "ofk_get_lk_light", "ofk_lk_pyr_light",
    "ofk_set_corner_grid", "ofk_get_corner_grid", "ofk_corner_grid_download", "ofk_select_corners_grid", "ofk_good_features_grid",
    "ofk_set_zones", "ofk_get_zones", "ofk_zones_step", "ofk_zones_reset", "ofk_zones_download",
    "ofk_set_camera", "ofk_get_camera", "ofk_undistort_points", "ofk_distort_points", "ofk_camera_download",
    "ofk_set_rolling_shutter", "ofk_get_rolling_shutter", "ofk_rs_correct_points", "ofk_rs_download",
    "ofk_set_finite_motion", "ofk_get_finite_motion", "ofk_finite_correct_points", "ofk_finite_download",
    "ofk_set_track_table", "ofk_get_track_table", "ofk_track_table_download", "ofk_track_table_step", "ofk_track_seed_points",
    "ofk_set_track_depth", "ofk_get_track_depth", "ofk_track_depth_download", "ofk_track_depth_reset", "ofk_track_depth_step",
    "ofk_set_keyframe", "ofk_get_keyframe", "ofk_keyframe_download", "ofk_keyframe_reset", "ofk_keyframe_step",
    "ofk_set_keyframe_rotation", "ofk_get_keyframe_rotation", "ofk_keyframe_rotation_download", "ofk_keyframe_rotation_step",
    "ofk_set_keyframe_map", "ofk_get_keyframe_map", "ofk_keyframe_map_download", "ofk_keyframe_map_step",
    "ofk_set_pos_filter", "ofk_get_pos_filter", "ofk_pos_filter_input", "ofk_pos_filter_reset", "ofk_pos_filter_download", "ofk_pos_filter_step",
    "ofk_set_stabilise", "ofk_get_stabilise", "ofk_stab_download", "ofk_stab_frames", "ofk_stab_reset", "ofk_stab_pose",
    "ofk_set_rectify", "ofk_get_rectify",
    "ofk_set_track_template", "ofk_get_track_template", "ofk_track_template_download", "ofk_track_affine_fit", "ofk_track_template_step",
    "ofk_post_solve", "ofk_kf_predict_update", "ofk_of_simulation", "ofk_of_simulation_rng", "ofk_noise_normals", "ofk_feas_simulation", "ofk_hist_overlap", "ofk_associate_sensors", "ofk_feature_eval", "ofk_d_split", "ofk_pairs_upload", "ofk_pairs_upload_jpeg", "ofk_jpeg_stage", "ofk_jpeg_stage_error", "ofk_pairs_upload_staged", "ofk_jpeg_info", "ofk_jpeg_destuff", "ofk_jpeg_decode_bgr8", "ofk_jpeg_last_iterations", "ofk_pairs_set_sensors",
    "ofk_pairs_run", "ofk_pairs_download", "ofk_pairs_export_records_f32", "ofk_stream_begin", "ofk_stream_step",
    "ofk_stream_begin_jpeg", "ofk_stream_step_jpeg",
    "ofk_set_streams", "ofk_set_overlap", "ofk_set_tuning", "ofk_get_tuning", "ofk_mark", "ofk_mark_wait", "ofk_profile_enable", "ofk_profile_read", "ofk_resident_pyramid",
    "ofk_imu_reset", "ofk_imu_push", "ofk_imu_state", "ofk_filter_configure", "ofk_filter_state", "ofk_stream_step_fused",
    "ofk_stream_step_fused_jpeg", "ofk_stream_last_points", "ofk_pairs_filter_step",
    "ofk_comm_unique_id", "ofk_comm_init", "ofk_comm_add", "ofk_comm_destroy", "ofk_comm_rank", "ofk_comm_world", "ofk_comm_gather_records",
    "ofk_comm_fetch_records", "ofk_comm_allreduce_f64", "ofk_comm_count", "ofk_comm_pending", "ofk_comm_reorder_records",
)


class OfkError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libofk error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    _fields_ = [("max_corners", C.c_int), ("quality", C.c_double), ("min_distance", C.c_double), ("block_size", C.c_int),
                ("win", C.c_int), ("max_level", C.c_int), ("max_count", C.c_int), ("eps", C.c_double),
                ("min_eig_thr", C.c_double), ("solve_variant", C.c_int), ("use_feasibility", C.c_int), ("feas_T", C.c_double)]


LK_USE_INITIAL_FLOW, LK_GET_MIN_EIGENVALS = 4, 8         # cv2's OPTFLOW_* values (ofk_lk_pyr_ex)
BORDER_CONSTANT, BORDER_REPLICATE = 0, 1                 # ofk_warp_perspective (cv2's BORDER_* values)
BORDERS = {"constant": BORDER_CONSTANT, "replicate": BORDER_REPLICATE}
SEED_OFF, SEED_MODEL, SEED_ROTATION = 0, 1, 2           # ofk_set_lk_seed / ofk_predict_points
SEED_MODES = {"off": SEED_OFF, "model": SEED_MODEL, "rotation": SEED_ROTATION}
ROBUST_OFF, ROBUST_HUBER, ROBUST_TUKEY = 0, 1, 2         # ofk_set_robust / ofk_velocity_solve_robust
ROBUST_LOSSES = {"off": ROBUST_OFF, "huber": ROBUST_HUBER, "tukey": ROBUST_TUKEY}
ROBUST_DEFAULT_C = {ROBUST_HUBER: 1.345, ROBUST_TUKEY: 4.685}     # 95 % efficiency on Gaussian residuals
ROBUST_MIN_POINTS, ROBUST_DOUBLES = 8, 8
COV_OFF, COV_PROPAGATE, COV_RESIDUAL = 0, 1, 2           # ofk_set_cov / ofk_velocity_solve_cov
COV_MODES = {"off": COV_OFF, "propagate": COV_PROPAGATE, "residual": COV_RESIDUAL}
COV_DOUBLES = 24
JOINT_OFF, JOINT_ON = 0, 1                               # ofk_set_joint / ofk_velocity_solve_joint
JOINT_DOUBLES = 32
BIAS_OFF, BIAS_ON = 0, 1                                 # ofk_set_gyro_bias / ofk_gyro_bias_step
BIAS_DOUBLES = 32
PLANE_OFF, PLANE_ON = 0, 1                               # ofk_set_plane / ofk_velocity_solve_plane
PLANE_DOUBLES = 32
EPI_OFF, EPI_ON = 0, 1                                   # ofk_set_epipolar / ofk_velocity_solve_epipolar
EPI_W_ONE, EPI_W_ROBUST = 0, 1
EPI_WEIGHTS = {"one": EPI_W_ONE, "robust": EPI_W_ROBUST}
EPI_DOUBLES = 32
EPI_SIGMA_MAX = 0.008                                    # radians; tests/test_epi_reference.py measures it
FB_OFF, FB_PLAIN, FB_SEEDED = 0, 1, 2                    # ofk_set_track_gate / ofk_lk_pyr_fb
FB_MODES = {"off": FB_OFF, "plain": FB_PLAIN, "seeded": FB_SEEDED}
LIGHT_OFF, LIGHT_BIAS, LIGHT_GAIN = 0, 1, 2              # ofk_set_lk_light / ofk_lk_pyr_light
LIGHT_MODES = {"off": LIGHT_OFF, "bias": LIGHT_BIAS, "gain": LIGHT_GAIN}
GRID_MAX_CELLS = 2048                                   # OFK_GRID_MAX_CELLS: cells of a corner grid over one frame
ZONES_OFF, ZONES_HULL = 0, 1                             # ofk_set_zones
ZONES_MODES = {"off": ZONES_OFF, "hull": ZONES_HULL}
ZONE_MAX, ZONE_VERTS, ZONE_INTS, ZONE_FLOATS, ZONE_STATS = 16, 32, 67, 4, 8    # OFK_ZONE_*: slots per stream, vertices per zone, the download's rows
CAMERA_OFF, CAMERA_BROWN, CAMERA_FISHEYE = 0, 1, 2       # ofk_set_camera / ofk_undistort_points / ofk_distort_points
CAMERA_MODELS = {"off": CAMERA_OFF, "brown": CAMERA_BROWN, "fisheye": CAMERA_FISHEYE}
CAMERA_DEFAULT_ITERS = {CAMERA_BROWN: 20, CAMERA_FISHEYE: 10}
RS_OFF, RS_FLOW, RS_GYRO = 0, 1, 2                       # ofk_set_rolling_shutter / ofk_rs_correct_points
RS_MODES = {"off": RS_OFF, "flow": RS_FLOW, "gyro": RS_GYRO}
RS_MAX_ROWS = 65536
FM_OFF, FM_EXACT = 0, 1                                  # ofk_set_finite_motion / ofk_finite_correct_points
FM_MODES = {"off": FM_OFF, "exact": FM_EXACT}
TT_OFF, TT_ON = 0, 1                                     # ofk_set_track_table
TT_SEED_OFF, TT_SEED_FLOW = 0, 1
TT_SEEDS = {"off": TT_SEED_OFF, "flow": TT_SEED_FLOW}
TT_STATS = 8                                             # count, kept, lost, born, oldest age, step, next_id, rows seeded from their flow
TD_OFF, TD_ON = 0, 1                                     # ofk_set_track_depth
TD_DOUBLES = 32                                          # v_map, flag, mature, updated, initialised, 3 skip counts, C_map, v, solved, reset
KEY_OFF, KEY_ON = 0, 1                                   # ofk_set_keyframe
KEY_DOUBLES, KEY_STATE, KEY_INTS = 32, 16, 4             # the record; R_acc, anchor, pos; key_step, members_at_key, keyframes, dead-reckoned steps
KEY_MIN_DEPTH = 0.1
KEY_SOLVED, KEY_UNSOLVED, KEY_NONE = 0, 1, 2             # the record's flag
KEY_RE_FLAG, KEY_RE_ROWS, KEY_RE_SHARE, KEY_RE_ANGLE, KEY_RE_AGE = 1, 2, 3, 4, 5   # the record's re-key reason
KEYROT_OFF, KEYROT_ON = 0, 1                             # ofk_set_keyframe_rotation
KEYROT_GYRO, KEYROT_ATTITUDE = 0, 1                      # where R_acc comes from
KEYROT_DOUBLES, KEYROT_STATE, KEYROT_MAX_ITERS = 40, 12, 8   # the record; R_world at the keyframe, valid, its key_step
KEYROT_OK, KEYROT_NONE, KEYROT_SINGULAR, KEYROT_LARGE, KEYROT_HELD = 0, 1, 2, 3, 4   # the record's flag
KEYMAP_OFF, KEYMAP_ON = 0, 1                             # ofk_set_keyframe_map
KEYMAP_DOUBLES = 32                                      # the record
KEYMAP_USED, KEYMAP_NONE, KEYMAP_FEW, KEYMAP_FELL_BACK = 0, 1, 2, 3   # the record's flag
KEY_RE_MAP = 6                                           # the keyframe record's re-key reason: depths that would give the keyframe a map
POSF_OFF, POSF_ON = 0, 1                                 # ofk_set_pos_filter
POSF_STATES, POSF_INPUT, POSF_INTS, POSF_DOUBLES = 12, 12, 16, 48   # x = (p, v, b, c); the input row; the counts; the record
POSF_NOT, POSF_APPLIED, POSF_GATED, POSF_REFUSED = 0, 1, 2, 3       # an update's outcome in the record
STAB_OFF, STAB_ROTATION, STAB_PLANE = 0, 1, 2            # ofk_set_stabilise
RECTIFY_OFF, RECTIFY_ON = 0, 1                           # ofk_set_rectify
STAB_MODES = {"off": STAB_OFF, "rotation": STAB_ROTATION, "plane": STAB_PLANE}
STAB_DOUBLES, STAB_INTS = 48, 4                          # the record; steps since the last re-base, re-bases, approx, a previous warp exists
STAB_NONE, STAB_ROTATION_ONLY, STAB_FULL = 0, 1, 2       # the record's flag
STAB_RB_COVER, STAB_RB_FINITE = 1, 2                     # the record's re-base reason
TPL_OFF, TPL_ON = 0, 1                                   # ofk_set_track_template
TPL_DOUBLES = 32                                         # M, t, fit flag, rows of the two fits, rms, nine counts, largest move
TPL_KEEP, TPL_DROP = 0, 1
TPL_OUTSIDE = {"keep": TPL_KEEP, "drop": TPL_DROP}
TPL_NOT_TRACKED, TPL_PASS, TPL_FAIL, TPL_ABANDONED, TPL_OUTSIDE_ROW, TPL_FLAT, TPL_NO_TEMPLATE, TPL_CAPTURED = 0, 1, 2, 3, 4, 5, 6, 16
FLOW_LK, FLOW_ROTATIONAL = 0, 1
KEEP_STATUS, KEEP_LEGACY = 0, 1
CONTROL_SENSORS, CONTROL_IMU = 0, 1


class Robust(C.Structure):
    """ofk_robust (include/ofk.h): the robust velocity solve's setting."""
    _fields_ = [("loss", C.c_int), ("c", C.c_double), ("iters", C.c_int), ("hypotheses", C.c_int), ("seed", C.c_ulonglong),
                ("drop", C.c_int)]


def robust_setting(loss="tukey", c=None, iters=5, hypotheses=64, seed=0, drop=False):
    """A Robust structure from names: loss "off" / "huber" / "tukey" (or ROBUST_*); c None = the loss's usual tuning constant."""
    if isinstance(loss, str):
        if loss not in ROBUST_LOSSES:
            raise ValueError(f"robust loss {loss!r} is none of {sorted(ROBUST_LOSSES)}")
        loss = ROBUST_LOSSES[loss]
    loss = int(loss)
    if c is None:
        c = ROBUST_DEFAULT_C.get(loss, ROBUST_DEFAULT_C[ROBUST_TUKEY])
    return Robust(loss, float(c), int(iters), int(hypotheses), int(seed) & 0xFFFFFFFFFFFFFFFF, int(bool(drop)))


def robust_pairs(seed, problem, hypotheses, m):
    """ofk_robust_pairs (host only): the kept-point numbers (i, j) of the hypotheses 0..hypotheses-1 of problem `problem`."""
    n = int(hypotheses)
    i = np.zeros(max(n, 1), np.int32); j = np.zeros(max(n, 1), np.int32)
    rc = load_library().ofk_robust_pairs(C.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint(int(problem)), n, int(m), _p(i), _p(j))
    if rc != 0:
        raise OfkError(rc, f"ofk_robust_pairs: hypotheses {n} outside 0..256 or m {m} < 2")
    return i[:max(n, 0)], j[:max(n, 0)]


class Cov(C.Structure):
    """ofk_cov (include/ofk.h): the velocity covariance's setting."""
    _fields_ = [("mode", C.c_int), ("sigma_flow", C.c_double), ("sigma_pos", C.c_double), ("sigma_d", C.c_double),
                ("sigma_omega", C.c_double * 3), ("sigma_normal", C.c_double), ("sigma_offset", C.c_double), ("omega_from_imu", C.c_int),
                ("filter_r", C.c_int), ("r_floor", C.c_double), ("nis_max", C.c_double)]


def cov_setting(mode="propagate", sigma_flow=0.0, sigma_pos=0.0, sigma_d=0.0, sigma_omega=0.0, sigma_normal=0.0, sigma_offset=0.0,
                omega_from_imu=False, filter_r=False, r_floor=0.0, nis_max=0.0):
    """A Cov structure from names: mode "off" / "propagate" / "residual" (or COV_*); sigma_omega a scalar or three values; sigma_flow
    and sigma_pos in the units of the points the entry takes (pixels in the resident paths)."""
    if isinstance(mode, str):
        if mode not in COV_MODES:
            raise ValueError(f"cov mode {mode!r} is none of {sorted(COV_MODES)}")
        mode = COV_MODES[mode]
    so = np.broadcast_to(np.asarray(sigma_omega, np.float64), (3,))
    return Cov(int(mode), float(sigma_flow), float(sigma_pos), float(sigma_d), (C.c_double * 3)(*so.tolist()), float(sigma_normal),
               float(sigma_offset), int(bool(omega_from_imu)), int(bool(filter_r)), float(r_floor), float(nis_max))


class Joint(C.Structure):
    """ofk_joint (include/ofk.h): the joint velocity and rotation solve's setting."""
    _fields_ = [("mode", C.c_int), ("sigma_flow", C.c_double), ("sigma_omega", C.c_double * 3), ("omega_from_imu", C.c_int)]


def joint_setting(mode=True, sigma_flow=0.2, sigma_omega=None, omega_from_imu=False):
    """A Joint structure from names: mode True / False (or JOINT_*); sigma_flow in the units of the points the entry takes (pixels in
    the resident paths); sigma_omega None = every axis free (+inf), a scalar or three values (+inf: free, 0: held)."""
    so = np.broadcast_to(np.asarray(np.inf if sigma_omega is None else sigma_omega, np.float64), (3,))
    return Joint(int(mode), float(sigma_flow), (C.c_double * 3)(*so.tolist()), int(bool(omega_from_imu)))


class GyroBias(C.Structure):
    """ofk_gyro_bias (include/ofk.h): the setting of a stream's gyro bias."""
    _fields_ = [("mode", C.c_int), ("sigma_flow", C.c_double), ("sigma_gyro", C.c_double), ("q", C.c_double), ("p0", C.c_double * 3),
                ("b0", C.c_double * 3), ("nis_max", C.c_double), ("update", C.c_int)]


def gyro_bias_setting(mode=True, sigma_flow=0.2, sigma_gyro=0.0, q=1e-12, p0=1e-2, b0=0.0, nis_max=0.0, update=True):
    """A GyroBias structure from names: mode True / False (or BIAS_*); sigma_flow in the units of the points the entry takes (pixels in
    the stream steps); sigma_gyro, p0 and b0 in rad per frame interval, q their variance per step; p0 and b0 a scalar or three values
    (p0 0: the axis is held at b0); nis_max 0 = no gate; update False applies b0 and never changes it."""
    p = np.broadcast_to(np.asarray(p0, np.float64), (3,)); b = np.broadcast_to(np.asarray(b0, np.float64), (3,))
    return GyroBias(int(mode), float(sigma_flow), float(sigma_gyro), float(q), (C.c_double * 3)(*p.tolist()), (C.c_double * 3)(*b.tolist()),
                    float(nis_max), int(bool(update)))


class Plane(C.Structure):
    """ofk_plane (include/ofk.h): the plane solve's setting."""
    _fields_ = [("mode", C.c_int), ("sigma_flow", C.c_double), ("sigma_normal", C.c_double), ("sigma_max", C.c_double),
                ("beam", C.c_double * 3), ("iters", C.c_int)]


def plane_setting(mode=True, sigma_flow=0.2, sigma_normal=None, sigma_max=0.1, beam=(0.0, 0.0, 1.0), iters=6):
    """A Plane structure from names: mode True / False (or PLANE_*); sigma_flow in the units of the points the entry takes (pixels in
    the resident paths); sigma_normal None = the tilt is free (+inf), else the prior's standard deviation in radians (0: held);
    sigma_max the largest predicted 1 sigma of the normal's angle that is accepted (radians, inf: no gate); beam the range sensor's
    direction in the camera frame; iters Gauss-Newton steps (1..16)."""
    b = np.broadcast_to(np.asarray(beam, np.float64), (3,))
    return Plane(int(mode), float(sigma_flow), float(np.inf if sigma_normal is None else sigma_normal), float(sigma_max),
                 (C.c_double * 3)(*b.tolist()), int(iters))


class Epipolar(C.Structure):
    """ofk_epipolar (include/ofk.h): the epipolar solve's setting."""
    _fields_ = [("mode", C.c_int), ("anchor", C.c_double), ("anchor_min", C.c_int), ("sigma_max", C.c_double), ("beam", C.c_double * 3),
                ("weights", C.c_int)]


def epipolar_setting(mode=True, anchor=np.inf, anchor_min=5, sigma_max=EPI_SIGMA_MAX, beam=(0.0, 0.0, 1.0), weights="one"):
    """An Epipolar structure from names: mode True / False (or EPI_*); anchor the radius around the beam's foot inside which the
    ground is the sensors' plane, in the units of the points the entry takes (pixels in the resident paths; inf: every kept point);
    anchor_min the fewest anchor points a scale is taken from; sigma_max the largest predicted 1 sigma of the direction that is
    accepted (radians, inf: no gate); beam the range sensor's direction in the camera frame; weights "one" / "robust" (or EPI_W_*)."""
    if isinstance(weights, str):
        if weights not in EPI_WEIGHTS:
            raise ValueError(f"epipolar weights {weights!r} is none of {sorted(EPI_WEIGHTS)}")
        weights = EPI_WEIGHTS[weights]
    b = np.broadcast_to(np.asarray(beam, np.float64), (3,))
    return Epipolar(int(mode), float(anchor), int(anchor_min), float(sigma_max), (C.c_double * 3)(*b.tolist()), int(weights))


def cov_matrix(t6):
    """The symmetric 3x3 of six record slots (xx xy xz yy yz zz); leading dimensions are kept."""
    t = np.asarray(t6, np.float64)
    return np.stack([t[..., [0, 1, 2]], t[..., [1, 3, 4]], t[..., [2, 4, 5]]], -2)


class TrackGate(C.Structure):
    """ofk_track_gate (include/ofk.h): the forward-backward check and the err cap behind LK."""
    _fields_ = [("fb_mode", C.c_int), ("fb_thr", C.c_double), ("fb_level", C.c_int), ("err_max", C.c_double)]


def track_gate_setting(fb="off", fb_thr=0.5, fb_level=-1, err_max=0.0):
    """A TrackGate structure from names: fb "off" / "plain" (the backward search starts at the forward result) / "seeded" (it starts
    at the original point), or FB_*; fb_thr in pixels; fb_level -1 = the forward pass's maxLevel; err_max 0 = no cap on LK's err."""
    if isinstance(fb, str):
        if fb not in FB_MODES:
            raise ValueError(f"track gate fb {fb!r} is none of {sorted(FB_MODES)}")
        fb = FB_MODES[fb]
    fb, fb_thr, fb_level, err_max = int(fb), float(fb_thr), int(fb_level), float(err_max)
    if fb not in FB_MODES.values():
        raise ValueError(f"track gate fb mode {fb} is none of FB_OFF, FB_PLAIN, FB_SEEDED")
    if fb != FB_OFF and not (np.isfinite(fb_thr) and fb_thr > 0.0):
        raise ValueError(f"track gate fb_thr {fb_thr} must be finite and positive")
    if fb_level < -1:
        raise ValueError(f"track gate fb_level {fb_level} must be -1 (the forward pass's) or a pyramid depth")
    if not (np.isfinite(err_max) and err_max >= 0.0):
        raise ValueError(f"track gate err_max {err_max} must be finite and not negative (0 = off)")
    return TrackGate(fb, fb_thr, fb_level, err_max)


class LkLight(C.Structure):
    """ofk_lk_light (include/ofk.h): the per-window gain and bias of the lighting-insensitive LK."""
    _fields_ = [("mode", C.c_int), ("gain_max", C.c_double)]


def lk_light_setting(mode="gain", gain_max=4.0):
    """An LkLight structure from names: mode "off" / "bias" (a brightness offset per window) / "gain" (a gain and an offset), or
    LIGHT_*; the gain is clamped to [1 / gain_max, gain_max]."""
    if isinstance(mode, str):
        if mode not in LIGHT_MODES:
            raise ValueError(f"lk light mode {mode!r} is none of {sorted(LIGHT_MODES)}")
        mode = LIGHT_MODES[mode]
    mode, gain_max = int(mode), float(gain_max)
    if mode not in LIGHT_MODES.values():
        raise ValueError(f"lk light mode {mode} is none of LIGHT_OFF, LIGHT_BIAS, LIGHT_GAIN")
    if not (np.isfinite(gain_max) and gain_max > 1.0):
        raise ValueError(f"lk light gain_max {gain_max} must be finite and above 1")
    return LkLight(mode, gain_max)


def _light(light):
    """None, a mode name or an LkLight -> an LkLight that is on, or None."""
    if light is None:
        return None
    m = lk_light_setting(light) if isinstance(light, (str, int)) and not isinstance(light, bool) else light
    if not isinstance(m, LkLight):
        raise ValueError(f"light {light!r} is neither None, a mode of {sorted(LIGHT_MODES)} nor an ofk.LkLight")
    m = lk_light_setting(m.mode, m.gain_max)                    # range-checked
    return None if m.mode == LIGHT_OFF else m


class CornerGrid(C.Structure):
    """ofk_corner_grid (include/ofk.h): the per-cell cap inside the greedy corner selection."""
    _fields_ = [("cell", C.c_int), ("cap", C.c_int), ("max_rank", C.c_int)]


def corner_grid_setting(cell=0, cap=0, max_rank=0):
    """A CornerGrid structure: cell = the cell edge in pixels (0 = off, the other fields are ignored then), cap = the most corners a
    cell may hold (>= 1), max_rank = 0 (every candidate may be examined) or the number of leading candidates the pass looks at."""
    cell, cap, max_rank = int(cell), int(cap), int(max_rank)
    if cell < 0:
        raise ValueError(f"corner grid cell {cell} must not be negative (0 = off)")
    if cell > 0 and cap < 1:
        raise ValueError(f"corner grid cap {cap} must be at least 1")
    if max_rank < 0:
        raise ValueError(f"corner grid max_rank {max_rank} must not be negative (0 = unlimited)")
    return CornerGrid(cell, cap, max_rank)


class Zones(C.Structure):
    """ofk_zones (include/ofk.h): the exclusion zones a stream builds from the points its solve stage rejected."""
    _fields_ = [("mode", C.c_int), ("link", C.c_int), ("min_members", C.c_int), ("radius", C.c_int), ("ttl", C.c_int), ("max_zones", C.c_int)]


def zones_setting(mode="hull", link=48, min_members=3, radius=20, ttl=30, max_zones=ZONE_MAX):
    """A Zones structure from names: mode "off" / "hull" (or ZONES_*); link = the per-axis distance in pixels below which two rejects
    belong to one cluster, min_members = the smallest cluster that becomes a zone, radius = the margin around the hull in pixels,
    ttl = the steps a zone lives without a refresh, max_zones = the slots in use (at most ZONE_MAX)."""
    if isinstance(mode, str):
        if mode not in ZONES_MODES:
            raise ValueError(f"zones mode {mode!r} is none of {sorted(ZONES_MODES)}")
        mode = ZONES_MODES[mode]
    mode, link, min_members, radius, ttl, max_zones = int(mode), int(link), int(min_members), int(radius), int(ttl), int(max_zones)
    if mode not in ZONES_MODES.values():
        raise ValueError(f"zones mode {mode} is neither ZONES_OFF nor ZONES_HULL")
    if mode != ZONES_OFF:
        for name, v, lo, hi in (("link", link, 1, 4096), ("min_members", min_members, 1, 4096), ("radius", radius, 0, 255), ("ttl", ttl, 1, 65535),
                                ("max_zones", max_zones, 1, ZONE_MAX)):
            if not lo <= v <= hi:
                raise ValueError(f"zones {name} {v} outside {lo}..{hi}")
    return Zones(mode, link, min_members, radius, ttl, max_zones)


class Camera(C.Structure):
    """ofk_camera (include/ofk.h): the lens model whose distortion is undone in front of the solve stage."""
    _fields_ = [("model", C.c_int), ("iters", C.c_int), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("k", C.c_double * 8), ("fo_x", C.c_double), ("fo_y", C.c_double), ("co_x", C.c_double), ("co_y", C.c_double)]


def camera_setting(model="brown", fx=1.0, fy=None, cx=0.0, cy=0.0, k=(), iters=None, fo_x=None, fo_y=None, co_x=None, co_y=None):
    """A Camera structure from names: model "off" / "brown" (cv2's pinhole model: k1 k2 p1 p2 [k3 [k4 k5 k6]]) / "fisheye" (cv2.fisheye,
    equidistant: k1..k4), or CAMERA_*; fx, fy, cx, cy = the camera matrix (fy None = fx); k = the coefficients in cv2's order, missing
    ones 0; fo_x, fo_y, co_x, co_y = the output matrix the ideal pixels are written in (None = fx for both focal lengths and the
    camera's centre: ONE focal length, as ofk_set_camera and the solve's one scaling ask for).

    iters is a fixed count; None = 20 for Brown and 10 for the fisheye, not cv2.undistortPoints' 5: on a strong wide-angle lens
    (k1 = -0.28, 1280 x 960, f = 1000) five fixed-point rounds leave up to 0.47 px of round-trip error at the frame's corners, 8 leave
    0.018 px, 10 leave 0.0021 px, 15 leave 1e-5 px and 20 leave 4e-8 px, while the fisheye's Newton iteration is at 5e-13 px after 3
    (tests/test_camera_reference.py pins the 5-round figure)."""
    if isinstance(model, str):
        if model not in CAMERA_MODELS:
            raise ValueError(f"camera model {model!r} is none of {sorted(CAMERA_MODELS)}")
        model = CAMERA_MODELS[model]
    model = int(model)
    if model not in CAMERA_MODELS.values():
        raise ValueError(f"camera model {model} is none of CAMERA_OFF, CAMERA_BROWN, CAMERA_FISHEYE")
    kk = [float(v) for v in np.asarray(k, np.float64).reshape(-1)]
    if len(kk) > 8:
        raise ValueError(f"camera k has {len(kk)} coefficients, more than 8")
    kk += [0.0] * (8 - len(kk))
    iters = CAMERA_DEFAULT_ITERS.get(model, 20) if iters is None else int(iters)
    fx = float(fx); fy = fx if fy is None else float(fy); cx = float(cx); cy = float(cy)
    fo_x = fx if fo_x is None else float(fo_x); fo_y = fo_x if fo_y is None else float(fo_y)
    co_x = cx if co_x is None else float(co_x); co_y = cy if co_y is None else float(co_y)
    if model != CAMERA_OFF:
        if not 1 <= iters <= 50:
            raise ValueError(f"camera iters {iters} outside 1..50")
        if not np.all(np.isfinite([fx, fy, cx, cy, fo_x, fo_y, co_x, co_y] + kk)):
            raise ValueError("camera: a field is not finite")
        if 0.0 in (fx, fy, fo_x, fo_y):
            raise ValueError("camera fx, fy, fo_x and fo_y must not be 0")
        if model == CAMERA_FISHEYE and any(kk[4:]):
            raise ValueError("camera: the fisheye model has four coefficients, k[4..7] must be 0")
    return Camera(model, iters, fx, fy, cx, cy, (C.c_double * 8)(*kk), fo_x, fo_y, co_x, co_y)


class RShutter(C.Structure):
    """ofk_rshutter (include/ofk.h): the rolling shutter whose per-row capture time is undone in front of the solve stage."""
    _fields_ = [("mode", C.c_int), ("rows", C.c_int), ("readout", C.c_double), ("anchor", C.c_double), ("omega_gain", C.c_double)]


def rshutter_setting(mode="gyro", readout=0.0, anchor=0.5, rows=0, omega_gain=1.0):
    """An RShutter structure from names: mode "off" / "flow" (constant image velocity from the measured flow, needs no sensor) /
    "gyro" (the rotation over the row time from the sensors' omega, exactly; the rest of the flow held constant), or RS_*;
    readout = the time from the first to the last row in frame intervals (negative: read from the bottom row up, |readout| <= 1);
    anchor = the row fraction in [0, 1] whose exposure the frame's time stamp belongs to; rows = the raw frame's row count (0 or
    None: the frame height of the run; the stage entry needs it > 0); omega_gain turns the sensors' omega into radians per frame
    interval (not 0)."""
    if isinstance(mode, str):
        if mode not in RS_MODES:
            raise ValueError(f"rolling-shutter mode {mode!r} is none of {sorted(RS_MODES)}")
        mode = RS_MODES[mode]
    mode = int(mode)
    if mode not in RS_MODES.values():
        raise ValueError(f"rolling-shutter mode {mode} is none of RS_OFF, RS_FLOW, RS_GYRO")
    rows = 0 if rows is None else int(rows)
    readout = float(readout); anchor = float(anchor); omega_gain = float(omega_gain)
    if mode != RS_OFF:
        if not np.all(np.isfinite([readout, anchor, omega_gain])):
            raise ValueError("rolling shutter: a field is not finite")
        if abs(readout) > 1.0:
            raise ValueError(f"rolling-shutter readout {readout} outside -1..1 frame intervals")
        if not 0.0 <= anchor <= 1.0:
            raise ValueError(f"rolling-shutter anchor {anchor} outside 0..1")
        if not 0 <= rows <= RS_MAX_ROWS:
            raise ValueError(f"rolling-shutter rows {rows} outside 0..{RS_MAX_ROWS}")
        if omega_gain == 0.0:
            raise ValueError("rolling-shutter omega_gain must not be 0")
    return RShutter(mode, rows, readout, anchor, omega_gain)


class FiniteMotion(C.Structure):
    """ofk_finite_motion (include/ofk.h): the frame pair's finite motion (exact rotation, plane displacement) written into the points
    in front of the solve stage."""
    _fields_ = [("mode", C.c_int), ("min_depth", C.c_double)]


def finite_motion_setting(mode="exact", min_depth=0.1):
    """A FiniteMotion structure from names: mode "off" / "exact", or FM_*; min_depth in (0, 1] = the smallest depth (in units of the
    previous depth) a point may have once the rotation is applied: below it the point keeps its place."""
    if isinstance(mode, str):
        if mode not in FM_MODES:
            raise ValueError(f"finite-motion mode {mode!r} is none of {sorted(FM_MODES)}")
        mode = FM_MODES[mode]
    mode = int(mode)
    if mode not in FM_MODES.values():
        raise ValueError(f"finite-motion mode {mode} is none of FM_OFF, FM_EXACT")
    min_depth = float(min_depth)
    if mode != FM_OFF and not (np.isfinite(min_depth) and 0.0 < min_depth <= 1.0):
        raise ValueError(f"finite-motion min_depth {min_depth} outside (0, 1]")
    return FiniteMotion(mode, min_depth)


class TrackTable(C.Structure):
    """ofk_track_table (include/ofk.h): an id, an age, a birth and the last flow per track of a stream, and LK seeded from that flow."""
    _fields_ = [("mode", C.c_int), ("seed", C.c_int), ("gain", C.c_double)]


def track_table_setting(seed="off", gain=1.0, mode=TT_ON):
    """A TrackTable structure from names: seed "off" / "flow" (or TT_SEED_*): LK starts at each track's position plus gain times its
    last flow; mode TT_ON / TT_OFF.  Newborn tracks have no flow: at a reduced pyramid depth they need lk_seed or slow motion."""
    mode = int(mode)
    if mode not in (TT_OFF, TT_ON):
        raise ValueError(f"track-table mode {mode} is none of TT_OFF, TT_ON")
    if isinstance(seed, str):
        if seed not in TT_SEEDS:
            raise ValueError(f"track-table seed {seed!r} is none of {sorted(TT_SEEDS)}")
        seed = TT_SEEDS[seed]
    seed = int(seed)
    if seed not in TT_SEEDS.values():
        raise ValueError(f"track-table seed {seed} is none of TT_SEED_OFF, TT_SEED_FLOW")
    gain = float(gain)
    if mode != TT_OFF and not np.isfinite(gain):
        raise ValueError(f"track-table gain {gain} must be finite")
    return TrackTable(mode, seed, gain)


class TrackDepth(C.Structure):
    """ofk_track_depth (include/ofk.h): an inverse depth per track of a stream, filtered over the frames, and the velocity from them."""
    _fields_ = [("mode", C.c_int), ("sigma_flow", C.c_double), ("b_min", C.c_double), ("gate", C.c_double), ("q", C.c_double),
                ("min_obs", C.c_int), ("rel_max", C.c_double), ("min_rows", C.c_int), ("update", C.c_int)]


def track_depth_setting(mode=True, sigma_flow=0.2, b_min=0.5, gate=3.0, q=0.0, min_obs=3, rel_max=0.25, min_rows=8, update=True):
    """A TrackDepth structure from names: mode True / False (or TD_*); sigma_flow and b_min in the units of the points the entry takes
    (pixels in the stream steps); gate in sigmas, on the cross-flow and on the innovation (0: no gates); q the variance a depth gains
    per step; a row is mature (enters the map solve) from min_obs measurements on with sqrt(var) <= rel_max * rho; the map solve needs
    min_rows (>= 3) mature rows; update False predicts the depths it has and takes no measurement into them."""
    mode = int(mode)
    if mode not in (TD_OFF, TD_ON):
        raise ValueError(f"track-depth mode {mode} is none of TD_OFF, TD_ON")
    t = TrackDepth(mode, float(sigma_flow), float(b_min), float(gate), float(q), int(min_obs), float(rel_max), int(min_rows), int(bool(update)))
    if mode != TD_OFF:
        if not all(np.isfinite(x) for x in (t.sigma_flow, t.b_min, t.gate, t.q, t.rel_max)):
            raise ValueError("track-depth sigma_flow, b_min, gate, q and rel_max must be finite")
        if not (t.sigma_flow > 0 and t.b_min >= 0 and t.gate >= 0 and t.q >= 0 and t.rel_max > 0 and t.min_obs >= 1 and t.min_rows >= 3):
            raise ValueError(f"track-depth setting outside its range: sigma_flow {t.sigma_flow} > 0, b_min {t.b_min} >= 0, gate {t.gate} >= 0, "
                             f"q {t.q} >= 0, min_obs {t.min_obs} >= 1, rel_max {t.rel_max} > 0, min_rows {t.min_rows} >= 3")
    return t


class Keyframe(C.Structure):
    """ofk_keyframe (include/ofk.h): the displacement of a stream against a frame that is held fixed."""
    _fields_ = [("mode", C.c_int), ("sigma_flow", C.c_double), ("gate", C.c_double), ("min_rows", C.c_int), ("min_share", C.c_double),
                ("rot_max", C.c_double), ("max_age", C.c_int)]


def keyframe_setting(mode=True, sigma_flow=0.2, gate=2.0, min_rows=8, min_share=0.5, rot_max=0.5, max_age=0):
    """A Keyframe structure from names: mode True / False (or KEY_*); sigma_flow and gate in pixels (gate 0: a single solve); the key
    solve needs min_rows (>= 3) rows; the keyframe is replaced when fewer than min_rows or fewer than min_share of its members are
    alive, when the accumulated rotation exceeds rot_max (rad) or when it is older than max_age steps (0: no limit)."""
    mode = int(mode)
    if mode not in (KEY_OFF, KEY_ON):
        raise ValueError(f"keyframe mode {mode} is none of KEY_OFF, KEY_ON")
    k = Keyframe(mode, float(sigma_flow), float(gate), int(min_rows), float(min_share), float(rot_max), int(max_age))
    if mode != KEY_OFF:
        if not all(np.isfinite(x) for x in (k.sigma_flow, k.gate, k.min_share, k.rot_max)):
            raise ValueError("keyframe sigma_flow, gate, min_share and rot_max must be finite")
        if not (k.sigma_flow > 0 and k.gate >= 0 and k.min_rows >= 3 and 0 <= k.min_share <= 1 and k.rot_max > 0 and k.max_age >= 0):
            raise ValueError(f"keyframe setting outside its range: sigma_flow {k.sigma_flow} > 0, gate {k.gate} >= 0, min_rows {k.min_rows} >= 3, "
                             f"min_share {k.min_share} in [0, 1], rot_max {k.rot_max} > 0, max_age {k.max_age} >= 0")
    return k


class TrackTemplate(C.Structure):
    """ofk_track_template (include/ofk.h): the birth patch per track of a stream, the score against it and the re-anchoring."""
    _fields_ = [("mode", C.c_int), ("win", C.c_int), ("ncc_min", C.c_double), ("anchor_iters", C.c_int), ("anchor_max", C.c_double),
                ("outside", C.c_int), ("fit_min", C.c_int), ("fit_gate", C.c_double), ("scale_max", C.c_double)]


def tpl_stride(win):
    """Bytes between the templates of two rows: (win + 2)^2 rounded up to a multiple of 4."""
    return ((int(win) + 2) ** 2 + 3) // 4 * 4


def track_template_setting(mode=True, win=15, ncc_min=0.8, anchor_iters=3, anchor_max=2.0, outside="keep", fit_min=6, fit_gate=2.0, scale_max=1.5):
    """A TrackTemplate structure from names: mode True / False (or TPL_*); win the odd template window (5..31); a row whose score
    against its template is below ncc_min is dropped; anchor_iters (0: score only) steps of at most anchor_max px in all pull the
    position back; outside "keep" / "drop" (or TPL_KEEP / TPL_DROP): rows whose window leaves the frame; the step map is fitted to at
    least fit_min rows, a second time over the rows within fit_gate px (0: once); a template is captured afresh when the accumulated
    map's area scale leaves [1 / scale_max^2, scale_max^2] (0: never)."""
    mode = int(mode)
    if mode not in (TPL_OFF, TPL_ON):
        raise ValueError(f"track-template mode {mode} is none of TPL_OFF, TPL_ON")
    if isinstance(outside, str):
        if outside not in TPL_OUTSIDE:
            raise ValueError(f"track-template outside {outside!r} is none of {sorted(TPL_OUTSIDE)}")
        outside = TPL_OUTSIDE[outside]
    t = TrackTemplate(mode, int(win), float(ncc_min), int(anchor_iters), float(anchor_max), int(outside), int(fit_min), float(fit_gate),
                      float(scale_max))
    if mode != TPL_OFF:
        if not all(np.isfinite(x) for x in (t.ncc_min, t.anchor_max, t.fit_gate, t.scale_max)):
            raise ValueError("track-template ncc_min, anchor_max, fit_gate and scale_max must be finite")
        if not (5 <= t.win <= 31 and t.win % 2 == 1 and -1 <= t.ncc_min <= 1 and 0 <= t.anchor_iters <= 8 and t.anchor_max > 0
                and t.outside in (TPL_KEEP, TPL_DROP) and t.fit_min >= 3 and t.fit_gate >= 0 and (t.scale_max == 0 or t.scale_max >= 1)):
            raise ValueError(f"track-template setting outside its range: win {t.win} odd in 5..31, ncc_min {t.ncc_min} in [-1, 1], "
                             f"anchor_iters {t.anchor_iters} in 0..8, anchor_max {t.anchor_max} > 0, outside {t.outside} in (0, 1), "
                             f"fit_min {t.fit_min} >= 3, fit_gate {t.fit_gate} >= 0, scale_max {t.scale_max} 0 or >= 1")
    return t


class KeyframeRotation(C.Structure):
    """ofk_keyframe_rotation (include/ofk.h): the keyframe's accumulated rotation refined from the flow."""
    _fields_ = [("mode", C.c_int), ("source", C.c_int), ("axes", C.c_int * 3), ("sigma_gyro", C.c_double), ("sigma_bias", C.c_double),
                ("sigma_att", C.c_double), ("iters", C.c_int), ("delta_max", C.c_double)]


def keyframe_rotation_setting(mode=True, source="gyro", axes=(1, 1, 1), sigma_gyro=0.0, sigma_bias=1e-4, sigma_att=1e-3, iters=2, delta_max=0.1):
    """A KeyframeRotation structure from names: mode True / False (or KEYROT_*); source "gyro" (R_acc is the product of the steps'
    rotations; prior variance age sigma_gyro^2 + (age sigma_bias)^2 per axis, in rad and rad per frame) or "attitude" (R_acc from
    R_world of the sensor rows; prior variance 2 sigma_att^2); axes: which of the three are estimated (0: held); iters Gauss-Newton
    steps; a correction beyond delta_max rad is refused."""
    mode = int(mode)
    if mode not in (KEYROT_OFF, KEYROT_ON):
        raise ValueError(f"keyframe-rotation mode {mode} is none of KEYROT_OFF, KEYROT_ON")
    src = {"gyro": KEYROT_GYRO, "attitude": KEYROT_ATTITUDE}.get(source, source)
    if src not in (KEYROT_GYRO, KEYROT_ATTITUDE):
        raise ValueError(f"keyframe-rotation source {source!r} is none of 'gyro', 'attitude'")
    ax = [int(bool(a)) for a in axes]
    if len(ax) != 3:
        raise ValueError("keyframe-rotation axes must be three flags")
    r = KeyframeRotation(mode, int(src), (C.c_int * 3)(*ax), float(sigma_gyro), float(sigma_bias), float(sigma_att), int(iters), float(delta_max))
    if mode != KEYROT_OFF:
        if not (r.sigma_gyro >= 0 and r.sigma_bias >= 0 and r.sigma_att >= 0 and np.isfinite(r.sigma_att) and 1 <= r.iters <= KEYROT_MAX_ITERS
                and r.delta_max > 0):
            raise ValueError(f"keyframe-rotation setting outside its range: sigma_gyro {r.sigma_gyro} >= 0, sigma_bias {r.sigma_bias} >= 0, "
                             f"sigma_att {r.sigma_att} finite >= 0, iters {r.iters} in 1..{KEYROT_MAX_ITERS}, delta_max {r.delta_max} > 0")
    return r


class KeyframeMap(C.Structure):
    """ofk_keyframe_map (include/ofk.h): the key solve against the per-track depths frozen at the keyframe."""
    _fields_ = [("mode", C.c_int), ("min_obs", C.c_int), ("rel_max", C.c_double), ("min_rows", C.c_int), ("ready_share", C.c_double),
                ("weights", C.c_int)]


def keyframe_map_setting(mode=True, min_obs=3, rel_max=0.02, min_rows=8, ready_share=0.5, weights=1):
    """A KeyframeMap structure from names: mode True / False (or KEYMAP_*); a depth enters the map with at least min_obs measurements
    and a sigma of at most rel_max of itself; the map is used with at least min_rows rows captured and alive; a keyframe without a
    map is replaced once ready_share of its live rows have such a depth (0: never); weights 1: each row weighted by its depth's
    variance times its parallax."""
    mode = int(mode)
    if mode not in (KEYMAP_OFF, KEYMAP_ON):
        raise ValueError(f"keyframe-map mode {mode} is none of KEYMAP_OFF, KEYMAP_ON")
    m = KeyframeMap(mode, int(min_obs), float(rel_max), int(min_rows), float(ready_share), int(weights))
    if mode != KEYMAP_OFF:
        if not (m.min_obs >= 1 and np.isfinite(m.rel_max) and m.rel_max > 0 and m.min_rows >= 3 and 0 <= m.ready_share <= 1 and m.weights in (0, 1)):
            raise ValueError(f"keyframe-map setting outside its range: min_obs {m.min_obs} >= 1, rel_max {m.rel_max} finite > 0, "
                             f"min_rows {m.min_rows} >= 3, ready_share {m.ready_share} in [0, 1], weights {m.weights} in (0, 1)")
    return m


class PosFilter(C.Structure):
    """ofk_pos_filter (include/ofk.h): keyframe displacement, velocity and position fixes fused in a filter with a cloned state."""
    _fields_ = [("mode", C.c_int), ("dt", C.c_double), ("sigma_v", C.c_double), ("floor", C.c_double), ("infl", C.c_double), ("share", C.c_double),
                ("q_p", C.c_double), ("q_v", C.c_double), ("q_b", C.c_double), ("p0_p", C.c_double), ("p0_v", C.c_double), ("p0_b", C.c_double),
                ("nis_max", C.c_double)]


def pos_filter_setting(mode=True, dt=1.0, sigma_v=1e-3, floor=0.0, infl=1.0, share=0.5, q_p=0.0, q_v=1e-3, q_b=0.0, p0_p=0.0, p0_v=1.0, p0_b=0.0,
                       nis_max=0.0):
    """A PosFilter structure from names: mode True / False (or POSF_*); dt: the step's length in the time unit of v; sigma_v: the
    sigma of v_uav as a velocity measurement (0: not used); the keyframe's D enters with C = infl^2 R_world C_T R_world^T + floor^2 I,
    of which `share` is the key pixels' part, added once per keyframe to the clone; q_p, q_v, q_b: process noise per step; p0_p,
    p0_v, p0_b: the prior's sigmas (a block with p0 = q = 0 is held); nis_max: an update whose NIS exceeds it is gated (0: none)."""
    mode = int(mode)
    if mode not in (POSF_OFF, POSF_ON):
        raise ValueError(f"position-filter mode {mode} is none of POSF_OFF, POSF_ON")
    f = PosFilter(mode, *[float(v) for v in (dt, sigma_v, floor, infl, share, q_p, q_v, q_b, p0_p, p0_v, p0_b, nis_max)])
    if mode != POSF_OFF:
        vals = [getattr(f, n) for n, _ in PosFilter._fields_[1:]]
        if not all(np.isfinite(v) for v in vals):
            raise ValueError("every field of the position-filter setting must be finite")
        if not (f.dt > 0 and f.infl > 0 and 0 <= f.share <= 1 and min(f.sigma_v, f.floor, f.q_p, f.q_v, f.q_b, f.p0_p, f.p0_v, f.p0_b, f.nis_max) >= 0):
            raise ValueError(f"position-filter setting outside its range: dt {f.dt} > 0, infl {f.infl} > 0, share {f.share} in [0, 1], "
                             f"sigma_v, floor, q_*, p0_* and nis_max >= 0")
    return f


class Stabilise(C.Structure):
    """ofk_stabilise (include/ofk.h): every step's new gray frame warped into the view of the stream's keyframe."""
    _fields_ = [("mode", C.c_int), ("border", C.c_int), ("border_value", C.c_int), ("min_cover", C.c_double), ("chain", C.c_int)]


def stabilise_setting(mode=True, border=BORDER_CONSTANT, border_value=0, min_cover=0.5, chain=1):
    """A Stabilise structure from names: mode True (the plane's homography) / False, "plane", "rotation" (R alone) or STAB_*; border
    "constant" / "replicate" or BORDER_*, with border_value 0..255 outside the frame; a view whose warp covered less than min_cover of
    the frame is re-based on the current keyframe (0: never); chain 1: the view stays the first keyframe's across re-keys, 0: it jumps
    to each new keyframe."""
    mode = STAB_MODES[mode] if isinstance(mode, str) else STAB_PLANE if mode is True else int(mode)
    if mode not in (STAB_OFF, STAB_ROTATION, STAB_PLANE):
        raise ValueError(f"stabilise mode {mode} is none of STAB_OFF, STAB_ROTATION, STAB_PLANE")
    m = Stabilise(mode, BORDERS[border] if isinstance(border, str) else int(border), int(border_value), float(min_cover), int(chain))
    if mode != STAB_OFF:
        if not (m.border in (BORDER_CONSTANT, BORDER_REPLICATE) and 0 <= m.border_value <= 255 and np.isfinite(m.min_cover) and 0 <= m.min_cover < 1
                and m.chain in (0, 1)):
            raise ValueError(f"stabilise setting outside its range: border {m.border} in (0, 1), border_value {m.border_value} in 0..255, "
                             f"min_cover {m.min_cover} in [0, 1), chain {m.chain} in (0, 1)")
    return m


class Rectify(C.Structure):
    """ofk_rectify (include/ofk.h): the stabilised view of a stream behind a lens, resampled through the lens's forward map."""
    _fields_ = [("mode", C.c_int), ("r_max", C.c_double)]


def rectify_setting(mode=True, r_max=0.0):
    """A Rectify structure from names: mode True / False or RECTIFY_*; r_max the largest ideal normalised radius that is sampled
    (0: no bound) - 1.05 * CameraModel.ideal_radius(h, w) keeps a folding Brown polynomial out of the view."""
    mode = RECTIFY_ON if mode is True else RECTIFY_OFF if mode is False else int(mode)
    if mode not in (RECTIFY_OFF, RECTIFY_ON):
        raise ValueError(f"rectify mode {mode} is neither RECTIFY_OFF nor RECTIFY_ON")
    r = Rectify(mode, float(r_max))
    if mode != RECTIFY_OFF and not (np.isfinite(r.r_max) and r.r_max >= 0):
        raise ValueError(f"rectify r_max {r.r_max} is negative or not finite")
    return r


class Fusion(C.Structure):
    """ofk_fusion (include/ofk.h): what ofk_stream_step_fused does between LK and the next frame."""
    _fields_ = [("use_imu", C.c_int), ("flow", C.c_int), ("keep", C.c_int), ("filter", C.c_int), ("control", C.c_int),
                ("z_sign", C.c_double), ("z_source", C.c_int), ("vel_overwrite", C.c_int), ("redetect_replace", C.c_int),
                ("min_solve", C.c_int), ("hold_on_skip", C.c_int)]


# the struct settings: ofk_set_<name> / ofk_get_<name> take the context and a pointer to the struct
SETTINGS = (("robust", Robust), ("cov", Cov), ("joint", Joint), ("gyro_bias", GyroBias), ("plane", Plane), ("epipolar", Epipolar), ("track_gate", TrackGate), ("lk_light", LkLight),
            ("corner_grid", CornerGrid), ("zones", Zones), ("camera", Camera), ("rolling_shutter", RShutter), ("finite_motion", FiniteMotion),
            ("track_table", TrackTable), ("track_depth", TrackDepth), ("track_template", TrackTemplate), ("keyframe", Keyframe),
            ("keyframe_rotation", KeyframeRotation), ("keyframe_map", KeyframeMap), ("pos_filter", PosFilter), ("stabilise", Stabilise), ("rectify", Rectify))

_lib = None
_lib_lock = threading.Lock()


def jpeg_info(stream):
    """(h, w, components) of a JPEG stream the device decoder accepts; OfkError otherwise (host-side header parse)."""
    data = bytes(stream)
    h, w, n = C.c_int(), C.c_int(), C.c_int()
    rc = load_library().ofk_jpeg_info(data, len(data), C.byref(h), C.byref(w), C.byref(n))
    if rc != 0:
        raise OfkError(rc, "not a JPEG stream the decoder supports (8-bit baseline Huffman, one interleaved scan, gray or YCbCr "
                           "4:4:4/4:2:2/4:2:0)")
    return h.value, w.value, n.value


def jpeg_destuff(stream):
    """(entropy segment without its byte stuffing and restart markers, offsets behind the removed RSTn markers) - what the ingest's
    staging hands to the device decoders (host only)."""
    data = bytes(stream)
    out = C.create_string_buffer(max(1, len(data)))
    rst = (C.c_uint32 * (len(data) // 2 + 1))()
    n, nr = C.c_size_t(), C.c_int()
    rc = load_library().ofk_jpeg_destuff(data, len(data), out, len(data), C.byref(n), rst, len(rst), C.byref(nr))
    if rc != 0:
        raise OfkError(rc, "ofk_jpeg_destuff: not a JPEG stream the decoder supports")
    return out.raw[:n.value], list(rst[:nr.value])


def load_library():
    """Loads libofk.so and declares the signatures.  Raises OfkError if the library is not built."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise OfkError(E_NOGPU, f"{LIB_PATH} not built (run `make -C {os.path.join(_HERE, 'csrc')}` or "
                                    "__graft_entry__.build()); there is no CPU fallback")
        # The resident pipeline keeps 4 HIP streams busy (2 free-running slices x {chain, auxiliary}) beside the caller's own
        # (torch's, RCCL's).  The HIP runtime multiplexes streams onto 4 hardware queues unless told otherwise, and two streams of
        # one queue run in order.  Only effective if the runtime is not initialised yet; a value the user set wins.
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
        L = C.CDLL(LIB_PATH)
        vp, i, d = C.c_void_p, C.c_int, C.c_double
        L.ofk_version.restype = i
        for name, cls in SETTINGS:
            getattr(L, "ofk_set_" + name).argtypes = getattr(L, "ofk_get_" + name).argtypes = [vp, C.POINTER(cls)]
        L.ofk_last_error.restype = C.c_char_p; L.ofk_last_error.argtypes = [vp]
        L.ofk_device_count.restype = i
        L.ofk_create.argtypes = [i, i, i, i, i, i, C.POINTER(vp)]
        L.ofk_destroy.argtypes = [vp]; L.ofk_sync.argtypes = [vp]
        L.ofk_gray_bgr8.argtypes = [vp, vp, i, i, i, vp]
        L.ofk_pyr_down_u8.argtypes = [vp, vp, i, i, i, vp]
        L.ofk_pyramid_u8.argtypes = [vp, vp, i, i, i, i, vp, C.POINTER(i)]
        L.ofk_scharr_s16.argtypes = [vp, vp, i, i, i, vp]
        L.ofk_warp_perspective.argtypes = [vp, vp, i, i, i, vp, vp, i, i, i, i, i, vp]
        L.ofk_warp_lens.argtypes = [vp, C.POINTER(Camera), vp, i, i, i, vp, vp, i, i, i, i, d, i, vp]
        L.ofk_mineig_response.argtypes = [vp, vp, i, i, i, i, vp]
        L.ofk_select_corners.argtypes = [vp, vp, vp, i, i, i, i, d, d, vp, vp]
        L.ofk_good_features.argtypes = [vp, vp, vp, i, i, i, i, d, d, i, vp, vp]
        L.ofk_lk_pyr.argtypes = [vp, vp, vp, i, i, i, vp, vp, i, i, i, i, d, d, vp, vp, vp]
        L.ofk_lk_pyr_ex.argtypes = [vp, vp, vp, i, i, i, vp, vp, i, i, i, i, d, d, vp, i, vp, vp, vp]
        L.ofk_predict_points.argtypes = [vp, vp, vp, i, i, vp, i, d, vp]
        L.ofk_set_lk_seed.argtypes = [vp, i, d]; L.ofk_get_lk_seed.argtypes = [vp, C.POINTER(i), C.POINTER(d)]
        L.ofk_flow_model.argtypes = [vp, vp, i, i, vp, vp, vp, vp, vp, vp]
        L.ofk_feasibility.argtypes = [vp, i, vp, vp, i, i, vp, vp, vp, vp, vp, vp, vp]
        L.ofk_velocity_solve.argtypes = [vp, i, vp, vp, vp, i, i, vp, vp, vp, vp, vp, vp]
        L.ofk_robust_download.argtypes = [vp, vp, i, vp]
        L.ofk_velocity_solve_robust.argtypes = [vp, i, vp, vp, vp, i, i, vp, vp, vp, vp, vp, C.POINTER(Robust), vp, vp, vp]
        L.ofk_robust_pairs.argtypes = [C.c_ulonglong, C.c_uint, i, i, vp, vp]
        L.ofk_cov_download.argtypes = [vp, vp]
        L.ofk_joint_download.argtypes = [vp, vp]
        L.ofk_velocity_solve_joint.argtypes = [vp, i, vp, vp, vp, i, i, vp, vp, vp, vp, vp, C.POINTER(Robust), C.POINTER(Joint), vp, vp]
        L.ofk_velocity_solve_cov.argtypes = [vp, i, vp, vp, vp, i, i, vp, vp, vp, vp, vp, C.POINTER(Robust), C.POINTER(Cov), vp, vp]
        L.ofk_gyro_bias_reset.argtypes = [vp, vp, i]; L.ofk_gyro_bias_download.argtypes = [vp, vp]
        L.ofk_gyro_bias_step.argtypes = [vp, i, vp, vp, vp, i, i, vp, vp, vp, vp, C.POINTER(Robust), C.POINTER(GyroBias), vp, vp]
        L.ofk_plane_download.argtypes = [vp, vp]
        L.ofk_velocity_solve_plane.argtypes = [vp, i, vp, vp, vp, i, i, vp, vp, vp, vp, vp, C.POINTER(Robust), C.POINTER(Plane), vp, vp]
        L.ofk_epipolar_download.argtypes = [vp, vp]; L.ofk_epipolar_points_download.argtypes = [vp, vp]
        L.ofk_velocity_solve_epipolar.argtypes = [vp, i, vp, vp, vp, i, i, vp, vp, vp, vp, vp, C.POINTER(Robust), C.POINTER(Epipolar), vp, vp, vp]
        L.ofk_track_gate_download.argtypes = [vp, vp, vp, vp, i, vp]
        L.ofk_corner_grid_download.argtypes = [vp, vp]
        L.ofk_select_corners_grid.argtypes = [vp, vp, vp, i, i, i, i, d, d, vp, vp, C.POINTER(CornerGrid), vp, vp, i]
        L.ofk_good_features_grid.argtypes = [vp, vp, vp, i, i, i, i, d, d, i, vp, vp, C.POINTER(CornerGrid), vp, vp, i]
        L.ofk_zones_step.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, i, vp, vp]
        L.ofk_zones_reset.argtypes = [vp, i]; L.ofk_zones_download.argtypes = [vp, vp, vp, vp]
        L.ofk_undistort_points.argtypes = [vp, C.POINTER(Camera), vp, vp, i, i, vp]
        L.ofk_distort_points.argtypes = [vp, C.POINTER(Camera), vp, vp, i, i, vp]
        L.ofk_camera_download.argtypes = [vp, vp, vp, i]
        L.ofk_rs_correct_points.argtypes = [vp, C.POINTER(RShutter), vp, vp, vp, vp, vp, i, i, vp, vp, vp]
        L.ofk_rs_download.argtypes = [vp, vp, vp, i]
        L.ofk_finite_correct_points.argtypes = [vp, C.POINTER(FiniteMotion), vp, vp, vp, i, i, vp, vp, vp]
        L.ofk_finite_download.argtypes = [vp, vp, vp, i]
        L.ofk_track_table_download.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, vp]
        L.ofk_track_table_step.argtypes = [vp, C.POINTER(TrackTable), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, vp, vp]
        L.ofk_track_seed_points.argtypes = [vp, vp, vp, i, i, vp, vp, d, i, vp]
        L.ofk_track_depth_download.argtypes = [vp, vp, vp, vp, i, vp]
        L.ofk_track_depth_reset.argtypes = [vp, i, vp, vp, vp, i]
        L.ofk_track_depth_step.argtypes = [vp, C.POINTER(TrackDepth), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, vp]
        L.ofk_keyframe_download.argtypes = [vp, vp, vp, i, vp, vp]
        L.ofk_keyframe_reset.argtypes = [vp, i, vp]
        L.ofk_keyframe_step.argtypes = [vp, C.POINTER(Keyframe), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, vp]
        L.ofk_keyframe_rotation_download.argtypes = [vp, vp]
        L.ofk_keyframe_rotation_step.argtypes = [vp, C.POINTER(Keyframe), C.POINTER(KeyframeRotation), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i,
                                                 i, i, vp, vp, vp]
        L.ofk_keyframe_map_download.argtypes = [vp, vp, vp, i, vp]
        L.ofk_keyframe_map_step.argtypes = [vp, C.POINTER(Keyframe), C.POINTER(KeyframeMap), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, vp,
                                            vp, vp, vp, vp, vp, vp, vp]
        L.ofk_pos_filter_input.argtypes = [vp, vp]
        L.ofk_pos_filter_reset.argtypes = [vp, i, vp]
        L.ofk_pos_filter_download.argtypes = [vp, vp, vp, vp, vp]
        L.ofk_pos_filter_step.argtypes = [vp, C.POINTER(PosFilter), vp, vp, vp, vp, vp, vp, vp, vp, i, vp]
        L.ofk_stab_download.argtypes = [vp, vp, vp, vp]
        L.ofk_stab_frames.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.ofk_stab_reset.argtypes = [vp, i]
        L.ofk_stab_pose.argtypes = [vp, C.POINTER(Stabilise), vp, vp, vp, vp, vp, i, i, vp, vp, i, vp]
        L.ofk_track_template_download.argtypes = [vp, vp, vp, vp, vp, vp, i, vp]
        L.ofk_track_affine_fit.argtypes = [vp, C.POINTER(TrackTemplate), vp, vp, vp, vp, i, i, i, i, vp, vp]
        L.ofk_track_template_step.argtypes = [vp, C.POINTER(TrackTemplate), vp, vp, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, vp]
        L.ofk_lk_pyr_fb.argtypes = [vp, vp, vp, i, i, i, vp, vp, i, i, i, i, d, d, vp, i, vp, vp, vp, C.POINTER(TrackGate), vp, vp, vp]
        L.ofk_lk_pyr_light.argtypes = L.ofk_lk_pyr_fb.argtypes + [C.POINTER(LkLight)]
        L.ofk_imu_propagate.argtypes = [vp, vp, vp, i]
        L.ofk_post_solve.argtypes = [vp, vp, vp, vp, vp, i, vp]
        L.ofk_associate_sensors.argtypes = [vp, vp, i, vp, vp, vp, i, vp, vp, i, vp, vp, vp]
        L.ofk_feature_eval.argtypes = [vp, vp, vp, vp, vp, vp, i, i, vp, vp, d, d, i, i, vp, vp, vp, vp, vp, vp, vp]
        L.ofk_d_split.argtypes = [vp, vp, vp, i, i, d, vp, vp, vp]
        L.ofk_kf_predict_update.argtypes = [vp, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i]
        L.ofk_of_simulation.argtypes = [vp, vp, vp, vp, vp, i, vp, i, vp, vp]
        L.ofk_of_simulation_rng.argtypes = [vp, vp, vp, vp, vp, i, C.c_ulonglong, C.c_uint, C.c_uint, i, vp, vp]
        L.ofk_noise_normals.argtypes = [vp, C.c_ulonglong, C.c_uint, C.c_uint, i, vp]
        L.ofk_feas_simulation.argtypes = [vp, vp, vp, vp, vp, i, vp, i, vp, vp, vp]
        L.ofk_hist_overlap.argtypes = [vp, vp, i, vp, i, i, C.POINTER(i)]
        L.ofk_pairs_upload.argtypes = [vp, vp, vp, i, i, i]
        L.ofk_pairs_upload_jpeg.argtypes = [vp, vp, vp, vp, vp, i]
        L.ofk_jpeg_stage.argtypes = [vp, i, vp, vp, i]; L.ofk_pairs_upload_staged.argtypes = [vp, i]
        L.ofk_jpeg_stage_error.restype = C.c_char_p; L.ofk_jpeg_stage_error.argtypes = [vp, i]
        L.ofk_jpeg_info.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
        L.ofk_jpeg_destuff.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), i, C.POINTER(i)]
        L.ofk_jpeg_decode_bgr8.argtypes = [vp, vp, vp, i, vp]
        L.ofk_jpeg_last_iterations.argtypes = [vp]
        L.ofk_pairs_set_sensors.argtypes = [vp, vp, i]
        L.ofk_pairs_run.argtypes = [vp, C.POINTER(Params)]
        L.ofk_pairs_download.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.ofk_pairs_export_records_f32.argtypes = [vp, vp, i]
        L.ofk_stream_begin.argtypes = [vp, vp, i, i, i, C.POINTER(Params), vp, vp]
        L.ofk_stream_step.argtypes = [vp, vp, vp, C.POINTER(Params), i, i, vp, vp, vp]
        L.ofk_stream_begin_jpeg.argtypes = [vp, vp, vp, i, C.POINTER(Params), vp, vp]
        L.ofk_stream_step_jpeg.argtypes = [vp, vp, vp, vp, C.POINTER(Params), i, i, vp, vp, vp]
        L.ofk_imu_reset.argtypes = [vp, vp, i]; L.ofk_imu_push.argtypes = [vp, vp, vp, i, i]; L.ofk_imu_state.argtypes = [vp, vp, vp, i]
        L.ofk_filter_configure.argtypes = [vp, i, i, i, vp, vp, vp, vp, vp, vp, vp, i]; L.ofk_filter_state.argtypes = [vp, vp, vp, i]
        L.ofk_stream_step_fused.argtypes = [vp, vp, vp, C.POINTER(Params), C.POINTER(Fusion), i, i, vp, vp, vp, vp]
        L.ofk_stream_step_fused_jpeg.argtypes = [vp, vp, vp, vp, C.POINTER(Params), C.POINTER(Fusion), i, i, vp, vp, vp, vp]
        L.ofk_stream_last_points.argtypes = [vp, vp, vp, i]
        L.ofk_pairs_filter_step.argtypes = [vp, d, i, i]
        L.ofk_set_streams.argtypes = [vp, i]
        L.ofk_set_overlap.argtypes = [vp, i]
        L.ofk_set_tuning.argtypes = [C.c_char_p, i]; L.ofk_get_tuning.argtypes = [C.c_char_p, C.POINTER(i)]
        L.ofk_mark.argtypes = [vp, i]; L.ofk_mark_wait.argtypes = [vp, i]
        L.ofk_profile_enable.argtypes = [vp, i]
        L.ofk_profile_read.argtypes = [vp, vp, vp]
        L.ofk_resident_pyramid.argtypes = [vp, i, i, vp, C.c_size_t]
        L.ofk_comm_unique_id.argtypes = [vp, i]; L.ofk_comm_init.argtypes = [vp, vp, i, i, i]; L.ofk_comm_add.argtypes = [vp, vp]; L.ofk_comm_destroy.argtypes = [vp]
        L.ofk_comm_rank.argtypes = [vp]; L.ofk_comm_world.argtypes = [vp]
        L.ofk_comm_gather_records.argtypes = [vp, i, i]; L.ofk_comm_fetch_records.argtypes = [vp, i, i, vp]
        L.ofk_comm_allreduce_f64.argtypes = [vp, vp, i, i]
        L.ofk_comm_count.argtypes = [vp]; L.ofk_comm_pending.argtypes = [vp, i]; L.ofk_comm_reorder_records.argtypes = [vp, i, i, i, vp]
        for s in SYMBOLS:
            if s not in ("ofk_last_error", "ofk_jpeg_stage_error"):      # the two that return a message, not a status
                getattr(L, s).restype = i
        _lib = L
        return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _arr(a, dtype, shape=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    if shape is not None and a.shape != tuple(shape):
        a = np.ascontiguousarray(np.broadcast_to(a, shape))
    return a


def _opt(a, dtype, shape):
    return None if a is None else _arr(a, dtype, shape)


def _point_arrays(arrays, counts, sensors, out, message):
    """What the point stage entries do with their arguments.  arrays: the inputs, [B,S,2] (or [S,2]: one image) f32 of one shape,
    message(*shapes) the ValueError text otherwise; counts [B] or None = every point; sensors [B,28] or None; out: per output an
    array to start from (copied) or None = zeros.  -> (single, inputs [B,S,2], counts, sensors, outputs [B,S,2])."""
    a = [_arr(x, np.float32) for x in arrays]
    single = a[0].ndim == 2
    if single:
        a = [x[None] for x in a]
    if a[0].ndim != 3 or a[0].shape[2] != 2 or any(x.shape != a[0].shape for x in a[1:]):
        raise ValueError(message(*[x.shape for x in a]))
    B, S = a[0].shape[:2]
    counts = _arr(S if counts is None else counts, np.int32, (B,))
    sensors = _opt(sensors, np.float64, (B, SENSOR_DOUBLES))
    outs = [np.zeros((B, S, 2), np.float32) if o is None else np.array(o, np.float32).reshape(B, S, 2) for o in out]
    return single, a, counts, sensors, outs


class Context:
    """One device + one HIP stream + all device buffers.  Calls are serialised by an internal lock
    (the C library is not thread-safe; rospy invokes callbacks from several threads)."""

    def __init__(self, device=0, max_w=1920, max_h=1080, max_batch=1, max_pts=512, max_level=3):
        self._L = load_library()
        self._h = C.c_void_p()
        self._lock = threading.RLock()
        rc = self._L.ofk_create(device, max_w, max_h, max_batch, max_pts, max_level, C.byref(self._h))
        if rc != OK:
            raise OfkError(rc, self._L.ofk_last_error(None).decode())
        self.device, self.max_w, self.max_h = device, max_w, max_h
        self.max_batch, self.max_pts, self.max_level = max_batch, max_pts, max_level
        self._resident = None

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.ofk_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc):
        if rc != OK:
            raise OfkError(rc, self._L.ofk_last_error(self._h).decode())

    def sync(self):
        with self._lock:
            self._ck(self._L.ofk_sync(self._h))

    def _set_struct(self, fn, value, settings, maker, lock):
        """ofk_set_*: the struct `value`, or maker(**settings), or without either NULL (off); lock: whether the call takes self._lock."""
        v = value if value is not None or not settings else maker(**settings)
        with self._lock if lock else contextlib.nullcontext():
            self._ck(fn(self._h, C.byref(v) if v is not None else None))

    def _get_struct(self, fn, cls):
        v = cls()
        self._ck(fn(self._h, C.byref(v)))
        return v

    def _rows(self, who, batch, call, *specs):
        """A download whose rows the library writes for the latest run, whatever `batch` says: zeroed [max_batch, *shape] buffers for
        specs = (shape, dtype), call(*pointers) under the lock, the first `batch` rows of each.  who: names the ValueError for a
        batch outside 0..max_batch (None: not checked)."""
        if who is not None and not 0 <= int(batch) <= self.max_batch:
            raise ValueError(f"{who}: batch {batch} outside 0..{self.max_batch}")
        bufs = [np.zeros((self.max_batch,) + tuple(shape), dtype) for shape, dtype in specs]
        with self._lock:
            self._ck(call(*[_p(b) for b in bufs]))
        return [b[:batch].copy() for b in bufs]

    def _track_download(self, name, batch, stride, rows, streams, keys):
        """ofk_<name>_download(rows..., stride, streams...) -> dict(zip(keys, arrays)): per (tail, dtype) of `rows` one [batch,stride,*tail]
        (stride None: max_pts; no rows: the call takes no stride), per (shape, dtype) of `streams` one [batch,*shape]."""
        who, S = name + "_download", ()
        if rows:
            S = (self.max_pts if stride is None else int(stride),)
            if S[0] < 1:
                raise ValueError(f"{who}: stride {S[0]}")
        fn, n = getattr(self._L, "ofk_" + who), len(rows)
        out = self._rows(who, self.max_batch if batch is None else int(batch), lambda *p: fn(self._h, *p[:n], *S, *p[n:]),
                         *[(S + tuple(tail), dtype) for tail, dtype in rows], *streams)
        return dict(zip(keys, out))

    @staticmethod
    def _stage_rows(who, arr, name, max_total=None, dtype=np.float32):
        """The first array of a per-track stage entry, [B, S >= 1, 2] -> (array, B, S, max_total or its default S)."""
        a = _arr(arr, dtype)
        if a.ndim != 3 or a.shape[2] != 2 or a.shape[1] < 1:
            raise ValueError(f"{who}: {name} {a.shape} is not [B, S >= 1, 2]")
        return a, a.shape[0], a.shape[1], a.shape[1] if max_total is None else int(max_total)

    def _points_download(self, fn, batch):
        """ofk_camera_download / ofk_rs_download / ofk_finite_download: (prev, next) [batch,max_pts,2] f32."""
        spec = ((self.max_pts, 2), np.float32)
        return tuple(self._rows(fn[4:], batch, lambda a, b: getattr(self._L, fn)(self._h, a, b, self.max_pts), spec, spec))

    # ------------------------------------------------------------------ image stages
    @staticmethod
    def _batched(img, nd):
        img = np.asarray(img)
        single = img.ndim == nd
        return (img[None] if single else img), single

    def gray_bgr8(self, bgr):
        bgr, single = self._batched(bgr, 3)
        bgr = _arr(bgr, np.uint8)
        B, h, w, ch = bgr.shape
        if ch != 3:
            raise ValueError("expected [..., h, w, 3] BGR")
        out = np.empty((B, h, w), np.uint8)
        with self._lock:
            self._ck(self._L.ofk_gray_bgr8(self._h, _p(bgr), B, h, w, _p(out)))
        return out[0] if single else out

    def pyr_down(self, src):
        src, single = self._batched(src, 2)
        src = _arr(src, np.uint8)
        B, h, w = src.shape
        out = np.empty((B, (h + 1) // 2, (w + 1) // 2), np.uint8)
        with self._lock:
            self._ck(self._L.ofk_pyr_down_u8(self._h, _p(src), B, h, w, _p(out)))
        return out[0] if single else out

    def pyramid(self, gray, max_level):
        """Levels 1..L of the pyramid calcOpticalFlowPyrLK builds: list of [B,h_l,w_l] uint8 arrays (a list of 2-D arrays for one image)."""
        gray, single = self._batched(gray, 2)
        gray = _arr(gray, np.uint8)
        B, h, w = gray.shape
        shapes, hh, ww = [], h, w
        for _ in range(int(max_level)):
            hh, ww = (hh + 1) // 2, (ww + 1) // 2
            shapes.append((hh, ww))
        total = sum(a * b for a, b in shapes)
        out = np.empty((B, max(total, 1)), np.uint8)
        built = C.c_int()
        with self._lock:
            self._ck(self._L.ofk_pyramid_u8(self._h, _p(gray), B, h, w, int(max_level), _p(out), C.byref(built)))
        levels, o = [], 0
        stride = sum(a * b for a, b in shapes[:built.value])
        flat = out.reshape(-1)[:B * stride].reshape(B, stride) if stride else out[:, :0]
        for (a, b) in shapes[:built.value]:
            lvl = flat[:, o:o + a * b].reshape(B, a, b)
            levels.append(lvl[0] if single else lvl)
            o += a * b
        return levels

    def scharr(self, gray):
        gray, single = self._batched(gray, 2)
        gray = _arr(gray, np.uint8)
        B, h, w = gray.shape
        out = np.empty((B, h, w, 2), np.int16)
        with self._lock:
            self._ck(self._L.ofk_scharr_s16(self._h, _p(gray), B, h, w, _p(out)))
        return out[0] if single else out

    def warp_perspective(self, src, M, dsize=None, border="constant", border_value=0):
        """ofk_warp_perspective: cv2's 5-bit bilinear warp with M mapping a DESTINATION pixel to a SOURCE pixel (ofk.h states the rule).
        M [3,3]: one image, src [h,w] or [h,w,C]; M [B,3,3]: src [B,h,w] or [B,h,w,C]; C is 1 or 3.  dsize (height, width) of the
        destination, default the source's.  border: "constant" / "replicate" or BORDER_*.  -> (dst in src's layout, covered): the
        pixels per image whose four taps lie inside the source, an int for one image, [B] int32 otherwise."""
        M = _arr(M, np.float64)
        single = M.shape == (3, 3)
        if single:
            M = M[None]
        if M.ndim != 3 or M.shape[1:] != (3, 3):
            raise ValueError(f"warp_perspective: M {M.shape} is neither [3,3] nor [B,3,3]")
        src = _arr(src, np.uint8)
        if single:
            src = src[None]
        if src.ndim not in (3, 4) or src.shape[0] != M.shape[0] or 0 in src.shape:
            raise ValueError(f"warp_perspective: src {src.shape} does not hold one [h,w] or [h,w,C] image per matrix ({M.shape[0]})")
        ch = src.shape[3] if src.ndim == 4 else 1
        if ch not in (1, 3):
            raise ValueError(f"warp_perspective: {ch} channels (1 or 3)")
        B, sh, sw = src.shape[:3]
        dh, dw = (sh, sw) if dsize is None else (int(dsize[0]), int(dsize[1]))
        if dh < 1 or dw < 1:
            raise ValueError(f"warp_perspective: dsize {dsize}")
        mode = BORDERS[border] if isinstance(border, str) else int(border)
        out = np.empty((B, dh, dw) + src.shape[3:], np.uint8)
        covered = np.zeros(B, np.int32)
        with self._lock:
            self._ck(self._L.ofk_warp_perspective(self._h, _p(src), sh, sw, ch, _p(M), _p(out), dh, dw, mode, int(border_value), B, _p(covered)))
        return (out[0], int(covered[0])) if single else (out, covered)

    def warp_lens(self, src, camera, M=None, dsize=None, border="constant", border_value=0, r_max=0.0):
        """ofk_warp_lens: the warp of raw images of `camera` (a Camera; fo_x != fo_y is accepted) through the lens's forward map, M
        mapping a DESTINATION pixel to an IDEAL pixel of the camera's output matrix (ofk.h states the rule).  Layouts as
        warp_perspective.  M None: the identity for every image, plain rectification (cv2.undistort); then src [h,w] or [h,w,3] is one
        image and [B,h,w,C] (or [B,h,w] with w != 3) a batch.  r_max: ideal normalised radius beyond which a pixel is border (0: no
        bound).  -> (dst in src's layout, covered)."""
        src = _arr(src, np.uint8)
        if M is None:
            single = src.ndim == 2 or (src.ndim == 3 and src.shape[2] == 3)
        else:
            M = _arr(M, np.float64)
            single = M.shape == (3, 3)
            if single:
                M = M[None]
            if M.ndim != 3 or M.shape[1:] != (3, 3):
                raise ValueError(f"warp_lens: M {M.shape} is neither [3,3] nor [B,3,3]")
        if single:
            src = src[None]
        if src.ndim not in (3, 4) or 0 in src.shape or (M is not None and src.shape[0] != M.shape[0]):
            raise ValueError(f"warp_lens: src {src.shape} does not hold one [h,w] or [h,w,C] image per matrix")
        ch = src.shape[3] if src.ndim == 4 else 1
        if ch not in (1, 3):
            raise ValueError(f"warp_lens: {ch} channels (1 or 3)")
        B, sh, sw = src.shape[:3]
        dh, dw = (sh, sw) if dsize is None else (int(dsize[0]), int(dsize[1]))
        if dh < 1 or dw < 1:
            raise ValueError(f"warp_lens: dsize {dsize}")
        mode = BORDERS[border] if isinstance(border, str) else int(border)
        out = np.empty((B, dh, dw) + src.shape[3:], np.uint8)
        covered = np.zeros(B, np.int32)
        with self._lock:
            self._ck(self._L.ofk_warp_lens(self._h, C.byref(camera), _p(src), sh, sw, ch, _p(M), _p(out), dh, dw, mode, int(border_value), float(r_max), B,
                                           _p(covered)))
        return (out[0], int(covered[0])) if single else (out, covered)

    def mineig(self, gray, block_size):
        gray, single = self._batched(gray, 2)
        gray = _arr(gray, np.uint8)
        B, h, w = gray.shape
        out = np.empty((B, h, w), np.float32)
        with self._lock:
            self._ck(self._L.ofk_mineig_response(self._h, _p(gray), B, h, w, int(block_size), _p(out)))
        return out[0] if single else out

    @staticmethod
    def _occupancy(occupied, B):
        """The occupancy list of a grid entry: None, or (points [B,S,2], counts [B]) -> (points f32 [B,S,2], counts i32 [B], S >= 1)."""
        if occupied is None:
            return None, None, 0
        pts, counts = occupied
        pts = _arr(pts, np.float32)
        pts = pts.reshape(B, -1, 2) if pts.size else np.zeros((B, 1, 2), np.float32)
        return np.ascontiguousarray(pts), _arr(counts, np.int32, (B,)), pts.shape[1]

    def select_corners(self, eig, max_corners, quality, min_distance, mask=None, grid=None, occupied=None):
        """grid: None = the context's setting (ofk_select_corners); a CornerGrid = ofk_select_corners_grid with that setting and
        `occupied` (None, or (points [B,S,2], counts [B])) as the occupancy list."""
        eig, single = self._batched(eig, 2)
        eig = _arr(eig, np.float32)
        B, h, w = eig.shape
        mask = _opt(mask, np.uint8, (B, h, w))
        pts = np.zeros((B, max_corners, 2), np.float32); cnt = np.zeros(B, np.int32)
        if grid is None and occupied is not None:
            raise ValueError("an occupancy list needs grid=")
        with self._lock:
            if grid is None:
                self._ck(self._L.ofk_select_corners(self._h, _p(eig), _p(mask), B, h, w, int(max_corners), float(quality),
                                                    float(min_distance), _p(pts), _p(cnt)))
            else:
                op, oc, S = self._occupancy(occupied, B)
                self._ck(self._L.ofk_select_corners_grid(self._h, _p(eig), _p(mask), B, h, w, int(max_corners), float(quality),
                                                         float(min_distance), _p(pts), _p(cnt), C.byref(grid), _p(op), _p(oc), S))
        return (pts[0], int(cnt[0])) if single else (pts, cnt)

    def good_features(self, gray, max_corners, quality, min_distance, block_size, mask=None, grid=None, occupied=None):
        """Batched goodFeaturesToTrack.  Returns (pts [B,max_corners,2] f32, counts [B]) or, for a single
        image, the OpenCV-shaped (N,1,2) float32 array.  grid / occupied: as in select_corners (ofk_good_features_grid)."""
        gray, single = self._batched(gray, 2)
        gray = _arr(gray, np.uint8)
        B, h, w = gray.shape
        mask = _opt(mask, np.uint8, (B, h, w))
        pts = np.zeros((B, max_corners, 2), np.float32); cnt = np.zeros(B, np.int32)
        if grid is None and occupied is not None:
            raise ValueError("an occupancy list needs grid=")
        with self._lock:
            if grid is None:
                self._ck(self._L.ofk_good_features(self._h, _p(gray), _p(mask), B, h, w, int(max_corners), float(quality),
                                                   float(min_distance), int(block_size), _p(pts), _p(cnt)))
            else:
                op, oc, S = self._occupancy(occupied, B)
                self._ck(self._L.ofk_good_features_grid(self._h, _p(gray), _p(mask), B, h, w, int(max_corners), float(quality),
                                                        float(min_distance), int(block_size), _p(pts), _p(cnt), C.byref(grid), _p(op), _p(oc), S))
        if single:
            n = int(cnt[0])
            return pts[0, :n].reshape(n, 1, 2).copy()
        return pts, cnt

    def lk_pyr(self, prev, nxt, prev_pts, counts=None, win=15, max_level=3, max_count=20, eps=0.03, min_eig_thr=1e-4, next_pts=None,
               flags=0, light=None):
        """Batched calcOpticalFlowPyrLK.  Single image: prev_pts (N,1,2)/(N,2) -> (next (N,1,2), status (N,1), err (N,1)).
        Batch: prev_pts [B,S,2] + counts [B] -> (next [B,S,2], status [B,S], err [B,S]).
        flags: LK_USE_INITIAL_FLOW (the search starts at next_pts, same shape as prev_pts) | LK_GET_MIN_EIGENVALS (err = level-0
        minEig); with flags == 0 and no next_pts this is ofk_lk_pyr, otherwise ofk_lk_pyr_ex.
        light: None, "bias", "gain" or an LkLight - the lighting-insensitive tracker, ofk_lk_pyr_light (only when given and on)."""
        flags = int(flags)
        light = _light(light)
        if flags & ~(LK_USE_INITIAL_FLOW | LK_GET_MIN_EIGENVALS):
            raise ValueError(f"lk_pyr: unknown flag bits {flags:#x}")
        if flags & LK_USE_INITIAL_FLOW and next_pts is None:
            raise ValueError("lk_pyr: LK_USE_INITIAL_FLOW needs next_pts")
        prev, single = self._batched(prev, 2)
        nxt, _ = self._batched(nxt, 2)
        prev = _arr(prev, np.uint8); nxt = _arr(nxt, np.uint8)
        if nxt.shape != prev.shape:
            raise ValueError(f"lk_pyr: next frame {nxt.shape} does not match the previous frame {prev.shape}")
        B, h, w = prev.shape
        if single:
            pp = _arr(prev_pts, np.float32).reshape(1, -1, 2)
            counts = np.array([pp.shape[1]], np.int32)
        else:
            pp = _arr(prev_pts, np.float32)
            counts = _arr(counts, np.int32, (B,))
        if pp.ndim != 3 or pp.shape[0] != B or pp.shape[2] != 2:
            raise ValueError(f"lk_pyr: prev_pts {pp.shape} is not [{B}, S, 2]")
        S = pp.shape[1]
        if np.any(counts < 0) or np.any(counts > S):
            raise ValueError("lk_pyr: counts outside 0..S")
        init = None
        if flags & LK_USE_INITIAL_FLOW:
            init = _arr(next_pts, np.float32)
            if init.size != pp.size:
                raise ValueError(f"lk_pyr: next_pts {init.shape} does not match prev_pts {pp.shape}")
            init = np.ascontiguousarray(init.reshape(pp.shape))
        if S == 0:
            z = np.zeros((0, 1, 2), np.float32)
            return z, np.zeros((0, 1), np.uint8), np.zeros((0, 1), np.float32)
        nxt_pts = np.zeros((B, S, 2), np.float32); st = np.zeros((B, S), np.uint8); err = np.zeros((B, S), np.float32)
        with self._lock:
            if light is not None:
                self._ck(self._L.ofk_lk_pyr_light(self._h, _p(prev), _p(nxt), B, h, w, _p(pp), _p(counts), S, int(win), int(max_level),
                                                  int(max_count), float(eps), float(min_eig_thr), _p(init) if init is not None else None,
                                                  flags, _p(nxt_pts), _p(st), _p(err), None, None, None, None, C.byref(light)))
            elif flags == 0:
                self._ck(self._L.ofk_lk_pyr(self._h, _p(prev), _p(nxt), B, h, w, _p(pp), _p(counts), S, int(win), int(max_level),
                                            int(max_count), float(eps), float(min_eig_thr), _p(nxt_pts), _p(st), _p(err)))
            else:
                self._ck(self._L.ofk_lk_pyr_ex(self._h, _p(prev), _p(nxt), B, h, w, _p(pp), _p(counts), S, int(win), int(max_level),
                                               int(max_count), float(eps), float(min_eig_thr), _p(init) if init is not None else None,
                                               flags, _p(nxt_pts), _p(st), _p(err)))
        if single:
            return nxt_pts[0].reshape(S, 1, 2), st[0].reshape(S, 1), err[0].reshape(S, 1)
        return nxt_pts, st, err

    def predict_points(self, pts, counts, sensors, mode=SEED_MODEL, gain=1.0):
        """ofk_predict_points: the start positions a seeded LK takes for pts [B,S,2] (counts [B]) under sensors [B,28]; entries
        beyond counts[b] are the points themselves.  Touches no resident state."""
        pp = _arr(pts, np.float32)
        if pp.ndim != 3 or pp.shape[2] != 2:
            raise ValueError(f"predict_points: pts {pp.shape} is not [B, S, 2]")
        B, S = pp.shape[:2]
        counts = _arr(counts, np.int32, (B,))
        sensors = _arr(sensors, np.float64, (B, SENSOR_DOUBLES))
        out = np.zeros((B, S, 2), np.float32)
        if S == 0:
            return out
        with self._lock:
            self._ck(self._L.ofk_predict_points(self._h, _p(pp), _p(counts), B, S, _p(sensors), _seed_mode(mode), float(gain), _p(out)))
        return out

    def set_lk_seed(self, mode, gain=1.0):
        """ofk_set_lk_seed: "off" / "model" / "rotation" (or SEED_*): every later pairs_run and stream step starts LK at the position
        the sensors predict."""
        self._ck(self._L.ofk_set_lk_seed(self._h, _seed_mode(mode), float(gain)))

    def get_lk_seed(self):
        m = C.c_int(0); g = C.c_double(0)
        self._ck(self._L.ofk_get_lk_seed(self._h, C.byref(m), C.byref(g)))
        return m.value, g.value

    def set_track_gate(self, gate=None, **settings):
        """ofk_set_track_gate: a TrackGate (or track_gate_setting's keywords); None switches both gates off.  Every later pairs_run
        and stream step clears the status of the points the gates reject, behind LK and in front of the solve."""
        self._set_struct(self._L.ofk_set_track_gate, gate, settings, track_gate_setting, lock=False)

    def get_track_gate(self):
        return self._get_struct(self._L.ofk_get_track_gate, TrackGate)

    def set_lk_light(self, light=None, **settings):
        """ofk_set_lk_light: an LkLight, a mode name (or lk_light_setting's keywords); None or mode "off" switches it off.  Every
        later pairs_run and stream step tracks with a gain and a bias per window taken out (the backward pass of a forward-backward
        gate too); everything behind LK sees only different next / status / err."""
        if isinstance(light, (str, int)):
            light = lk_light_setting(light, **settings); settings = {}
        self._set_struct(self._L.ofk_set_lk_light, light, settings, lk_light_setting, lock=True)

    def get_lk_light(self):
        return self._get_struct(self._L.ofk_get_lk_light, LkLight)

    def set_corner_grid(self, grid=None, **settings):
        """ofk_set_corner_grid: a CornerGrid (or corner_grid_setting's keywords); None switches the grid off.  Every later corner
        selection of the context (good_features, select_corners, pairs_run, stream begin and re-detection) caps the corners per cell."""
        self._set_struct(self._L.ofk_set_corner_grid, grid, settings, corner_grid_setting, lock=True)

    def get_corner_grid(self):
        return self._get_struct(self._L.ofk_get_corner_grid, CornerGrid)

    def corner_grid_stats(self, batch):
        """ofk_corner_grid_download: [batch,2] int32 = (corners accepted, candidates examined) per image of the latest selection with
        a grid on.  The library writes that selection's rows, so the buffer has max_batch of them and the first `batch` are returned."""
        return self._rows("corner_grid_stats", batch, lambda st: self._L.ofk_corner_grid_download(self._h, st), ((2,), np.int32))[0]

    def set_zones(self, zones=None, **settings):
        """ofk_set_zones: a Zones (or zones_setting's keywords); None or mode "off" switches the feature off.  Every later stream
        step feeds the points its solve stage rejected into the stream's zone table and keeps its re-detection out of the zones;
        pairs_run ignores the setting."""
        self._set_struct(self._L.ofk_set_zones, zones, settings, zones_setting, lock=True)

    def get_zones(self):
        return self._get_struct(self._L.ofk_get_zones, Zones)

    def set_track_table(self, track_table=None, **settings):
        """ofk_set_track_table: a TrackTable (or track_table_setting's keywords); None or mode TT_OFF switches it off.  Every later
        stream begin and step keeps an id, an age, a birth and the last flow per track on the device; with seed "flow" LK starts
        at each track's position plus its last flow.  pairs_run ignores the setting."""
        self._set_struct(self._L.ofk_set_track_table, track_table, settings, track_table_setting, lock=True)

    def get_track_table(self):
        return self._get_struct(self._L.ofk_get_track_table, TrackTable)

    def track_table_download(self, batch=None, stride=None):
        """ofk_track_table_download -> dict(ids, step_ids [batch,stride] u32, age, birth_step [batch,stride] i32, birth_xy, flow_xy
        [batch,stride,2] f32, stats [batch,8] i32: count, kept, lost, born, oldest age, step, next_id, rows seeded from their flow) of
        the streams of the latest begin or step with the setting on.  Rows are in the order of the tracks that call returned; the
        first stats[:, 0] of a stream are its tracks."""
        u, n, f = ((), np.uint32), ((), np.int32), ((2,), np.float32)
        return self._track_download("track_table", batch, stride, (u, n, n, f, f, u), [((TT_STATS,), np.int32)],
                                    ("ids", "age", "birth_step", "birth_xy", "flow_xy", "step_ids", "stats"))

    def track_table_step(self, table, head, prev_pts, next_pts, status, counts, new_pts=None, new_counts=None, max_total=None,
                         track_table=None):
        """ofk_track_table_step, the stage entry: one update of the table on host arrays.  table: dict(ids, age, birth_step [B,S],
        birth_xy, flow_xy [B,S,2]); head [B,2] = step, next_id; prev_pts / next_pts [B,S,2], status [B,S], counts [B]; new_pts [B,S,2]
        / new_counts [B] the re-detected corners (None: none); max_total (default S); track_table: the setting whose seed and gain the
        last statistic takes.  -> (table, head, counts, step_ids [B,S], stats [B,8]), new arrays.  Touches no resident state."""
        pp, B, S, mt = self._stage_rows("track_table_step", prev_pts, "prev_pts", max_total)
        pn = _arr(next_pts, np.float32, (B, S, 2)); st = _arr(status, np.uint8, (B, S))
        cn = np.array(_arr(counts, np.int32, (B,)))
        ids = np.array(_arr(table["ids"], np.uint32, (B, S))); age = np.array(_arr(table["age"], np.int32, (B, S)))
        bs = np.array(_arr(table["birth_step"], np.int32, (B, S)))
        bxy = np.array(_arr(table["birth_xy"], np.float32, (B, S, 2))); fxy = np.array(_arr(table["flow_xy"], np.float32, (B, S, 2)))
        hd = np.array(_arr(head, np.int32, (B, 2)))
        if (new_pts is None) != (new_counts is None):
            raise ValueError("track_table_step: new_pts and new_counts come together")
        nw = _opt(new_pts, np.float32, (B, S, 2)); nc = _opt(new_counts, np.int32, (B,))
        sid = np.zeros((B, S), np.uint32); stats = np.zeros((B, TT_STATS), np.int32)
        with self._lock:
            self._ck(self._L.ofk_track_table_step(self._h, C.byref(track_table) if track_table is not None else None, _p(ids), _p(age), _p(bs),
                                                  _p(bxy), _p(fxy), _p(hd), _p(pp), _p(pn), _p(st), _p(cn), _p(nw), _p(nc), mt, B, S, _p(sid), _p(stats)))
        return dict(ids=ids, age=age, birth_step=bs, birth_xy=bxy, flow_xy=fxy), hd, cn, sid, stats

    def track_seed_points(self, pts, counts, age, flow_xy, gain=1.0, seed=None):
        """ofk_track_seed_points, the stage entry: LK's start positions for pts [B,S,2] (counts [B]) from the tracks' age [B,S] and
        last flow [B,S,2].  seed: the model seeds [B,S,2] that rows of age 0 keep (None: they start at the point).  Entries beyond
        counts[b] are the points (or `seed`).  Touches no resident state."""
        pp, B, S, _ = self._stage_rows("track_seed_points", pts, "pts")
        cn = _arr(counts, np.int32, (B,)); ag = _arr(age, np.int32, (B, S)); fl = _arr(flow_xy, np.float32, (B, S, 2))
        out = np.array(pp if seed is None else _arr(seed, np.float32, (B, S, 2)))
        with self._lock:
            self._ck(self._L.ofk_track_seed_points(self._h, _p(pp), _p(cn), B, S, _p(ag), _p(fl), float(gain), 0 if seed is None else 1, _p(out)))
        return out

    def set_track_depth(self, track_depth=None, **settings):
        """ofk_set_track_depth: a TrackDepth (or track_depth_setting's keywords); None or mode False switches it off.  Every later
        stream step filters an inverse depth per row of the track table (which must be on) and solves v_map from the depths of the
        earlier frames.  pairs_run ignores the setting."""
        self._set_struct(self._L.ofk_set_track_depth, track_depth, settings, track_depth_setting, lock=True)

    def get_track_depth(self):
        return self._get_struct(self._L.ofk_get_track_depth, TrackDepth)

    def track_depth_download(self, batch=None, stride=None):
        """ofk_track_depth_download -> dict(rho, var [batch,stride] f64, nobs [batch,stride] i32, rec [batch,32]) of the streams of the
        latest step with the setting on, rows in the order of the tracks that step returned.  rec: v_map 0-2, map flag 3, mature rows
        4, rows updated 5, initialised 6, skipped for |b| 7, cross-flow 8, innovation 9, C_map's upper triangle 10-15, the v the
        measurements read 16-18, solved 19, rows reset 20."""
        f = ((), np.float64)
        return self._track_download("track_depth", batch, stride, (f, f, ((), np.int32)), [((TD_DOUBLES,), np.float64)], ("rho", "var", "nobs", "rec"))

    def track_depth_reset(self, stream, rho, var, nobs):
        """ofk_track_depth_reset: the first len(rho) rows of active stream `stream` are loaded from rho, var, nobs."""
        rho = _arr(rho, np.float64).ravel()
        var = _arr(var, np.float64, rho.shape); nobs = _arr(nobs, np.int32, rho.shape)
        with self._lock:
            self._ck(self._L.ofk_track_depth_reset(self._h, int(stream), _p(rho), _p(var), _p(nobs), len(rho)))

    def track_depth_step(self, x, u, status, counts, omega, v, solved, state, new_counts=None, max_total=None, track_depth=None, **settings):
        """ofk_track_depth_step, the stage entry: one step of the depths on host arrays.  x, u [B,S,2] f64 in the units of the setting;
        status [B,S], counts [B]; omega, v [B,3]; solved [B]; state: dict(rho, var [B,S] f64, nobs [B,S] i32); new_counts [B] the
        re-detected corners (None: none); max_total (default S); the setting a TrackDepth or track_depth_setting's keywords.
        -> (state, rec [B,32]), new arrays.  Touches no resident state."""
        td = track_depth if track_depth is not None else track_depth_setting(**settings)
        xx, B, S, mt = self._stage_rows("track_depth_step", x, "x", max_total, np.float64)
        uu = _arr(u, np.float64, (B, S, 2)); st = _arr(status, np.uint8, (B, S)); cn = _arr(counts, np.int32, (B,))
        om = _arr(omega, np.float64, (B, 3)); vv = _arr(v, np.float64, (B, 3)); so = _arr(solved, np.int32, (B,))
        rho = np.array(_arr(state["rho"], np.float64, (B, S))); var = np.array(_arr(state["var"], np.float64, (B, S)))
        nobs = np.array(_arr(state["nobs"], np.int32, (B, S)))
        nc = _opt(new_counts, np.int32, (B,))
        rec = np.zeros((B, TD_DOUBLES), np.float64)
        with self._lock:
            self._ck(self._L.ofk_track_depth_step(self._h, C.byref(td), _p(xx), _p(uu), _p(st), _p(cn), _p(om), _p(vv), _p(so), _p(rho), _p(var),
                                                  _p(nobs), _p(nc), mt, B, S, _p(rec)))
        return dict(rho=rho, var=var, nobs=nobs), rec

    def set_track_template(self, track_template=None, **settings):
        """ofk_set_track_template: a TrackTemplate (or track_template_setting's keywords); None or mode False switches it off.  Every
        later stream step keeps the birth patch of every row of the track table (which must be on), scores the tracked window against
        it through the accumulated map and pulls the position back onto it.  pairs_run ignores the setting."""
        self._set_struct(self._L.ofk_set_track_template, track_template, settings, track_template_setting, lock=True)

    def get_track_template(self):
        return self._get_struct(self._L.ofk_get_track_template, TrackTemplate)

    def track_template_download(self, batch=None, stride=None):
        """ofk_track_template_download -> dict(tmpl [batch,stride,tpl_stride(win)] u8, A [batch,stride,4] f32, ncc [batch,stride] f32,
        flag, tstate [batch,stride] u8, rec [batch,32]) of the streams of the latest step with the setting on, rows in the order of the
        tracks that step returned.  rec: M 0-3, t 4-5, fit flag 6, rows of the two fits 7-8, rms 9, rows scored 10, dropped 11, moved 12,
        abandoned 13, outside 14, flat 15, captured 16, without a template 17, marked for refresh 18, largest move 19."""
        u = ((), np.uint8)
        return self._track_download("track_template", batch, stride, (((tpl_stride(self.get_track_template().win),), np.uint8), ((4,), np.float32),
                                    ((), np.float32), u, u), [((TPL_DOUBLES,), np.float64)], ("tmpl", "A", "ncc", "flag", "tstate", "rec"))

    def track_affine_fit(self, prev_pts, next_pts, status, counts, h, w, track_template=None, **settings):
        """ofk_track_affine_fit, the stage entry of the templates' step map: prev_pts, next_pts [B,S,2] f32, status [B,S], counts [B],
        the frame's h and w -> (rec [B,32] with slots 0-9 filled, L [B,4] f32)."""
        tp = track_template if track_template is not None else track_template_setting(**settings)
        pp, B, S, _ = self._stage_rows("track_affine_fit", prev_pts, "prev_pts")
        nn = _arr(next_pts, np.float32, (B, S, 2)); st = _arr(status, np.uint8, (B, S)); cn = _arr(counts, np.int32, (B,))
        rec = np.zeros((B, TPL_DOUBLES), np.float64); L = np.zeros((B, 4), np.float32)
        with self._lock:
            self._ck(self._L.ofk_track_affine_fit(self._h, C.byref(tp), _p(pp), _p(nn), _p(st), _p(cn), B, S, int(h), int(w), _p(rec), _p(L)))
        return rec, L

    def track_template_step(self, prev, next, prev_pts, next_pts, status, age, counts, L, state, new_counts=None, max_total=None,
                            track_template=None, **settings):
        """ofk_track_template_step, the stage entry of rules 2-6 on host arrays: prev, next [B,h,w] u8 gray; prev_pts, next_pts [B,S,2]
        f32; status [B,S]; age [B,S] i32; counts [B]; L [B,4] f32 (track_affine_fit's); state: dict(tmpl [B,S,tpl_stride(win)] u8,
        A [B,S,4] f32, ncc [B,S] f32, flag, tstate [B,S] u8); new_counts [B] the re-detected corners (None: none); max_total (default
        S).  -> (next_pts, status: rows as tracked; state: compacted; rec [B,32] with slots 10-19 filled), new arrays.  Touches no
        resident state."""
        tp = track_template if track_template is not None else track_template_setting(**settings)
        g0 = _arr(prev, np.uint8)
        if g0.ndim != 3:
            raise ValueError(f"track_template_step: prev {g0.shape} is not [B, h, w]")
        B, h, w = g0.shape
        g1 = _arr(next, np.uint8, (B, h, w))
        pp = _arr(prev_pts, np.float32)
        if pp.ndim != 3 or pp.shape[0] != B or pp.shape[2] != 2 or pp.shape[1] < 1:
            raise ValueError(f"track_template_step: prev_pts {pp.shape} is not [{B}, S >= 1, 2]")
        S, ts = pp.shape[1], tpl_stride(tp.win)
        nn = np.array(_arr(next_pts, np.float32, (B, S, 2))); st = np.array(_arr(status, np.uint8, (B, S)))
        ag = _arr(age, np.int32, (B, S)); cn = _arr(counts, np.int32, (B,)); LL = _arr(L, np.float32, (B, 4))
        tm = np.array(_arr(state["tmpl"], np.uint8, (B, S, ts))); A = np.array(_arr(state["A"], np.float32, (B, S, 4)))
        ncc = np.array(_arr(state["ncc"], np.float32, (B, S))); fl = np.array(_arr(state["flag"], np.uint8, (B, S)))
        tst = np.array(_arr(state["tstate"], np.uint8, (B, S)))
        nc = _opt(new_counts, np.int32, (B,))
        rec = np.zeros((B, TPL_DOUBLES), np.float64)
        with self._lock:
            self._ck(self._L.ofk_track_template_step(self._h, C.byref(tp), _p(g0), _p(g1), h, w, _p(pp), _p(nn), _p(st), _p(ag), _p(cn), _p(LL),
                                                     _p(tm), _p(A), _p(ncc), _p(fl), _p(tst), _p(nc), S if max_total is None else int(max_total),
                                                     B, S, _p(rec)))
        return nn, st, dict(tmpl=tm, A=A, ncc=ncc, flag=fl, tstate=tst), rec

    def set_keyframe(self, keyframe=None, **settings):
        """ofk_set_keyframe: a Keyframe (or keyframe_setting's keywords); None or mode False switches it off.  Every later stream step
        solves the stream's displacement against a keyframe of its track table (which must be on) and reports a position that does
        not drift with the flow.  pairs_run ignores the setting."""
        self._set_struct(self._L.ofk_set_keyframe, keyframe, settings, keyframe_setting, lock=True)

    def get_keyframe(self):
        return self._get_struct(self._L.ofk_get_keyframe, Keyframe)

    def keyframe_download(self, batch=None, stride=None):
        """ofk_keyframe_download -> dict(key_xy [batch,stride,2] f32, member [batch,stride] u8, R_acc [batch,3,3], rec [batch,32]) of the
        streams of the latest step with the setting on, rows in the order of the tracks that step returned.  rec: T 0-2, flag 3, rows
        of the first / the gated solve 4 / 5, rms px 6, members_at_key 7, key_step 8, re-key reason 9, D 10-12, pos 13-15, anchor
        16-18, angle 19, C_T's upper triangle 20-25, keyframes 26, dead-reckoned steps 27, live 28, gated 29, the reasons as bits 30."""
        return self._track_download("keyframe", batch, stride, (((2,), np.float32), ((), np.uint8)), [((3, 3), np.float64), ((KEY_DOUBLES,), np.float64)],
                                    ("key_xy", "member", "R_acc", "rec"))

    def keyframe_reset(self, stream, anchor=None):
        """ofk_keyframe_reset: active stream `stream` starts over at the position `anchor` (None: zero) and keys at its next step."""
        a = None if anchor is None else _arr(anchor, np.float64, (3,))
        with self._lock:
            self._ck(self._L.ofk_keyframe_reset(self._h, int(stream), _p(a)))

    def set_keyframe_rotation(self, rotation=None, **settings):
        """ofk_set_keyframe_rotation: a KeyframeRotation (or keyframe_rotation_setting's keywords); None or mode False switches it off.
        Every later stream step with ofk_set_keyframe on (it must be) solves the keyframe's translation together with a correction of
        the accumulated rotation, under a prior from the source's sigmas."""
        self._set_struct(self._L.ofk_set_keyframe_rotation, rotation, settings, keyframe_rotation_setting, lock=True)

    def get_keyframe_rotation(self):
        return self._get_struct(self._L.ofk_get_keyframe_rotation, KeyframeRotation)

    def keyframe_rotation_download(self, batch=None):
        """ofk_keyframe_rotation_download -> rec [batch,40] of the streams of the latest step with the setting on: delta 0-2, flag 3
        (KEYROT_*), R^ 4-12, C_delta's upper triangle 13-18, C_T's 19-24, the reduced system's eigenvalues 25-27, the prior's sigmas
        28-30, Gauss-Newton steps 31, the plain first solve's T 32-34, attitude source used 35, age 36, rows 37."""
        return self._track_download("keyframe_rotation", batch, None, (), [((KEYROT_DOUBLES,), np.float64)], ("rec",))["rec"]

    def _keyframe_step(self, who, kf, rot, next_pts, status, counts, sensors, v_uav, solved, step, state, new_counts, max_total):
        nn, B, S, mt = self._stage_rows(who, next_pts, "next_pts", max_total)
        st = _arr(status, np.uint8, (B, S)); cn = _arr(counts, np.int32, (B,)); sn = _arr(sensors, np.float64, (B, SENSOR_DOUBLES))
        vu = _arr(v_uav, np.float64, (B, 3)); so = _arr(solved, np.int32, (B,)); sp = _arr(step, np.int32, (B,))
        kx = np.array(_arr(state["key_xy"], np.float32, (B, S, 2))); mem = np.array(_arr(state["member"], np.uint8, (B, S)))
        sd = np.array(_arr(state["state"], np.float64, (B, KEY_STATE))); si = np.array(_arr(state["istate"], np.int32, (B, KEY_INTS)))
        nc = _opt(new_counts, np.int32, (B,))
        rec = np.zeros((B, KEY_DOUBLES), np.float64)
        if rot is None:
            with self._lock:
                self._ck(self._L.ofk_keyframe_step(self._h, C.byref(kf), _p(nn), _p(st), _p(cn), _p(sn), _p(vu), _p(so), _p(sp), _p(kx), _p(mem),
                                                   _p(sd), _p(si), _p(nc), mt, B, S, _p(rec)))
            return dict(key_xy=kx, member=mem, state=sd, istate=si), rec
        rs = np.zeros((B, KEYROT_STATE), np.float64) if state.get("rstate") is None else np.array(_arr(state["rstate"], np.float64, (B, KEYROT_STATE)))
        rrec = np.zeros((B, KEYROT_DOUBLES), np.float64)
        with self._lock:
            self._ck(self._L.ofk_keyframe_rotation_step(self._h, C.byref(kf), C.byref(rot), _p(nn), _p(st), _p(cn), _p(sn), _p(vu), _p(so), _p(sp),
                                                        _p(kx), _p(mem), _p(sd), _p(si), _p(nc), mt, B, S, _p(rec), _p(rs), _p(rrec)))
        return dict(key_xy=kx, member=mem, state=sd, istate=si, rstate=rs), rec, rrec

    def keyframe_step(self, next_pts, status, counts, sensors, v_uav, solved, step, state, new_counts=None, max_total=None, keyframe=None,
                      **settings):
        """ofk_keyframe_step, the stage entry: rules 1-5 on host arrays.  next_pts [B,S,2] f32 ideal next points; status [B,S], counts
        [B]; sensors [B,28]; v_uav [B,3], solved [B] of the step's record; step [B] the table's step; state: dict(key_xy [B,S,2] f32,
        member [B,S] u8, state [B,16] f64, istate [B,4] i32); new_counts [B] the re-detected corners (None: none); max_total (default
        S); the setting a Keyframe or keyframe_setting's keywords.  -> (state, rec [B,32]), new arrays.  Touches no resident state."""
        kf = keyframe if keyframe is not None else keyframe_setting(**settings)
        return self._keyframe_step("keyframe_step", kf, None, next_pts, status, counts, sensors, v_uav, solved, step, state, new_counts, max_total)

    def keyframe_rotation_step(self, next_pts, status, counts, sensors, v_uav, solved, step, state, new_counts=None, max_total=None,
                               keyframe=None, rotation=None):
        """ofk_keyframe_rotation_step, the stage entry: keyframe_step's arguments; state may carry rstate [B,12] f64 (absent: zero, no
        R_world at the keyframe); keyframe: a Keyframe (None: the defaults), rotation: a KeyframeRotation (None: the defaults).
        -> (state with rstate, rec [B,32], rrec [B,40]), new arrays.  Touches no resident state."""
        kf = keyframe if keyframe is not None else keyframe_setting()
        rot = rotation if rotation is not None else keyframe_rotation_setting()
        return self._keyframe_step("keyframe_rotation_step", kf, rot, next_pts, status, counts, sensors, v_uav, solved, step, state, new_counts,
                                   max_total)

    def set_keyframe_map(self, keyframe_map=None, **settings):
        """ofk_set_keyframe_map: a KeyframeMap (or keyframe_map_setting's keywords); None or mode False switches it off.  Every later
        stream step with ofk_set_keyframe and ofk_set_track_depth on (both must be) freezes the depths at each keyframe and solves the
        key translation against them instead of the ground plane.  pairs_run ignores the setting."""
        self._set_struct(self._L.ofk_set_keyframe_map, keyframe_map, settings, keyframe_map_setting, lock=True)

    def get_keyframe_map(self):
        return self._get_struct(self._L.ofk_get_keyframe_map, KeyframeMap)

    def keyframe_map_download(self, batch=None, stride=None):
        """ofk_keyframe_map_download -> dict(key_rho, key_var [batch,stride] f64, rec [batch,32]) of the streams of the latest step with
        the setting on, rows in the order of the tracks that step returned.  rec: flag 0 (KEYMAP_*), map_rows 1, live map rows 2, rows
        of the first / the gated map solve 3 / 4, sum of weights 5, spread px 6, the plain first solve's T 7-9, rows captured this
        step 10, captured_for 11."""
        f = ((), np.float64)
        return self._track_download("keyframe_map", batch, stride, (f, f), [((KEYMAP_DOUBLES,), np.float64)], ("key_rho", "key_var", "rec"))

    def keyframe_map_step(self, next_pts, status, counts, sensors, v_uav, solved, step, state, depth=None, new_counts=None, max_total=None,
                          keyframe=None, keyframe_map=None):
        """ofk_keyframe_map_step, the stage entry: keyframe_step's arguments; state also carries key_rho, key_var [B,S] f64 and mstate
        [B,2] i32 (absent: zero); depth: dict(rho, var [B,S] f64, nobs [B,S] i32) as the previous depth step left it (None: no depth
        state); keyframe: a Keyframe (None: the defaults), keyframe_map: a KeyframeMap (None: the defaults).
        -> (state with key_rho, key_var, mstate; rec [B,32]; mrec [B,32]), new arrays.  Touches no resident state."""
        who = "keyframe_map_step"
        kf = keyframe if keyframe is not None else keyframe_setting()
        km = keyframe_map if keyframe_map is not None else keyframe_map_setting()
        nn, B, S, mt = self._stage_rows(who, next_pts, "next_pts", max_total)
        st = _arr(status, np.uint8, (B, S)); cn = _arr(counts, np.int32, (B,)); sn = _arr(sensors, np.float64, (B, SENSOR_DOUBLES))
        vu = _arr(v_uav, np.float64, (B, 3)); so = _arr(solved, np.int32, (B,)); sp = _arr(step, np.int32, (B,))
        kx = np.array(_arr(state["key_xy"], np.float32, (B, S, 2))); mem = np.array(_arr(state["member"], np.uint8, (B, S)))
        sd = np.array(_arr(state["state"], np.float64, (B, KEY_STATE))); si = np.array(_arr(state["istate"], np.int32, (B, KEY_INTS)))
        own = lambda name, dtype, shape: np.zeros(shape, dtype) if state.get(name) is None else np.array(_arr(state[name], dtype, shape))
        kr = own("key_rho", np.float64, (B, S)); kv = own("key_var", np.float64, (B, S)); ms = own("mstate", np.int32, (B, 2))
        rho = var = nobs = None
        if depth is not None:
            rho = _arr(depth["rho"], np.float64, (B, S)); var = _arr(depth["var"], np.float64, (B, S)); nobs = _arr(depth["nobs"], np.int32, (B, S))
        nc = _opt(new_counts, np.int32, (B,))
        rec = np.zeros((B, KEY_DOUBLES), np.float64); mrec = np.zeros((B, KEYMAP_DOUBLES), np.float64)
        with self._lock:
            self._ck(self._L.ofk_keyframe_map_step(self._h, C.byref(kf), C.byref(km), _p(nn), _p(st), _p(cn), _p(sn), _p(vu), _p(so), _p(sp), _p(kx),
                                                   _p(mem), _p(sd), _p(si), _p(nc), mt, B, S, _p(rec), _p(rho), _p(var), _p(nobs), _p(kr), _p(kv),
                                                   _p(ms), _p(mrec)))
        return dict(key_xy=kx, member=mem, state=sd, istate=si, key_rho=kr, key_var=kv, mstate=ms), rec, mrec

    def set_pos_filter(self, pos_filter=None, **settings):
        """ofk_set_pos_filter: a PosFilter (or pos_filter_setting's keywords); None or mode False switches it off.  Every later stream
        step with ofk_set_keyframe on (it must be) runs the stream's position filter behind the keyframe's step.  pairs_run ignores it."""
        self._set_struct(self._L.ofk_set_pos_filter, pos_filter, settings, pos_filter_setting, lock=True)

    def get_pos_filter(self):
        return self._get_struct(self._L.ofk_get_pos_filter, PosFilter)

    def set_stabilise(self, stabilise=None, **settings):
        """ofk_set_stabilise: a Stabilise (or stabilise_setting's keywords); None or mode False switches it off.  Every later stream
        step leaves the step's new gray frame warped into the keyframe's view on the device (stab_download)."""
        self._set_struct(self._L.ofk_set_stabilise, stabilise, settings, stabilise_setting, lock=True)

    def get_stabilise(self):
        return self._get_struct(self._L.ofk_get_stabilise, Stabilise)

    def set_rectify(self, rectify=None, **settings):
        """ofk_set_rectify: a Rectify (or rectify_setting's keywords); None or mode False switches it off.  With it and set_camera on,
        a stream step with set_stabilise on is accepted and warps its raw frame through the lens's map into the ideal view."""
        self._set_struct(self._L.ofk_set_rectify, rectify, settings, rectify_setting, lock=True)

    def get_rectify(self):
        return self._get_struct(self._L.ofk_get_rectify, Rectify)

    def stab_reset(self, stream):
        """ofk_stab_reset: the view of active stream `stream` starts over at the identity with its next step."""
        with self._lock:
            self._ck(self._L.ofk_stab_reset(self._h, int(stream)))

    def stab_download(self, batch=None, h=None, w=None, frames=True):
        """ofk_stab_download -> dict(frames [batch,h,w] u8 (frames=True; h, w: the streams' frame), rec [batch,48], covered [batch] i32) of
        the streams of the latest step with the setting on.  rec: M 0-8 (view pixel -> frame pixel), Bv 9-17, R 18-26, T 27-29, flag 30
        (STAB_*), re-base reason 31, steps since the last re-base 32, re-bases 33, approx 34, re-keyed 35, the previous cover 36."""
        B = self.max_batch if batch is None else int(batch)
        if not 0 <= B <= self.max_batch:
            raise ValueError(f"stab_download: batch {batch} outside 0..{self.max_batch}")
        rec = np.zeros((self.max_batch, STAB_DOUBLES), np.float64)
        cov = np.zeros(self.max_batch, np.int32)
        fr = None
        if frames:
            if h is None or w is None or int(h) * int(w) > self.max_w * self.max_h or int(h) < 1 or int(w) < 1:
                raise ValueError(f"stab_download: frames need the streams' h, w (got {h}, {w})")
            fr = np.zeros((self.max_batch, int(h), int(w)), np.uint8)
        with self._lock:
            self._ck(self._L.ofk_stab_download(self._h, _p(fr), _p(rec), _p(cov)))
        out = dict(rec=rec[:B].copy(), covered=cov[:B].copy())
        if frames:
            out["frames"] = fr[:B].copy()
        return out

    def stab_frames(self):
        """ofk_stab_frames -> (device pointer of the stabilised frames, bytes between images), for consumers on the device."""
        ptr, stride = C.c_void_p(), C.c_size_t()
        with self._lock:
            self._ck(self._L.ofk_stab_frames(self._h, C.byref(ptr), C.byref(stride)))
        return ptr.value, stride.value

    def stab_pose(self, R, key_rec, sensors, h, w, state=None, normal=None, prev_covered=None, stabilise=None, **settings):
        """ofk_stab_pose, the stage entry: rules 1-4 on host arrays.  R [B,3,3] the rotation the key solve used; key_rec [B,32] the
        keyframe's records; sensors [B,28]; h, w the frame; state: dict(Bv [B,3,3], ints [B,4]) of the previous call (None: the
        identity, zero); normal [B,3] (None: the sensor rows'); prev_covered [B] the previous warp's covered counts (read where
        ints[:, 3] != 0); the setting a Stabilise or stabilise_setting's keywords.  -> (state, rec [B,48]), new arrays."""
        st = stabilise if stabilise is not None else stabilise_setting(**settings)
        Rm = _arr(R, np.float64)
        if Rm.ndim != 3 or Rm.shape[1:] != (3, 3) or Rm.shape[0] < 1:
            raise ValueError(f"stab_pose: R {Rm.shape} is not [B >= 1, 3, 3]")
        B = Rm.shape[0]
        kr = _arr(key_rec, np.float64, (B, KEY_DOUBLES)); sn = _arr(sensors, np.float64, (B, SENSOR_DOUBLES))
        nr = _opt(normal, np.float64, (B, 3)); pc = _opt(prev_covered, np.int32, (B,))
        state = state or {}
        Bv = np.tile(np.eye(3), (B, 1, 1)) if state.get("Bv") is None else np.array(_arr(state["Bv"], np.float64, (B, 3, 3)))
        ints = np.zeros((B, STAB_INTS), np.int32) if state.get("ints") is None else np.array(_arr(state["ints"], np.int32, (B, STAB_INTS)))
        rec = np.zeros((B, STAB_DOUBLES), np.float64)
        with self._lock:
            self._ck(self._L.ofk_stab_pose(self._h, C.byref(st), _p(Rm), _p(kr), _p(sn), _p(nr), _p(pc), int(h), int(w), _p(Bv), _p(ints), B, _p(rec)))
        return dict(Bv=Bv, ints=ints), rec

    def pos_filter_input(self, input):
        """ofk_pos_filter_input: input [active streams, 12] f64 for the next step that is not held: du 0-2, fix valid 3, the fix 4-6, its
        sigmas 7-9."""
        a = _arr(input, np.float64)
        if a.ndim != 2 or a.shape[1] != POSF_INPUT or a.shape[0] > self.max_batch:
            raise ValueError(f"pos_filter_input: input {a.shape} is not [streams <= {self.max_batch}, {POSF_INPUT}]")
        full = np.zeros((self.max_batch, POSF_INPUT), np.float64)    # the library reads a row per active stream
        full[:len(a)] = a
        with self._lock:
            self._ck(self._L.ofk_pos_filter_input(self._h, _p(full)))

    def pos_filter_reset(self, stream, pos=None):
        """ofk_pos_filter_reset: active stream `stream` starts over at the position `pos` (None: zero) with its next step."""
        a = None if pos is None else _arr(pos, np.float64, (3,))
        with self._lock:
            self._ck(self._L.ofk_pos_filter_reset(self._h, int(stream), _p(a)))

    def pos_filter_download(self, batch=None):
        """ofk_pos_filter_download -> dict(x [batch,12], P [batch,12,12], istate [batch,16] i32, rec [batch,48]) of the streams of the
        latest step with the setting on.  rec: x 0-11, P_pp's upper triangle 12-17, P_vv's 18-23, trace of P_bb 24, per update
        (velocity 25-29, displacement 30-34, fix 35-39) outcome, NIS, innovation; cloned 40, fresh 41, steps 42, clones 43, updates
        applied / gated / refused 44-46, started this step 47."""
        x, P, ist, rec = self._rows("pos_filter_download", self.max_batch if batch is None else int(batch),
                                    lambda *p: self._L.ofk_pos_filter_download(self._h, *p), ((POSF_STATES,), np.float64),
                                    ((POSF_STATES, POSF_STATES), np.float64), ((POSF_INTS,), np.int32), ((POSF_DOUBLES,), np.float64))
        return dict(x=x, P=P, istate=ist, rec=rec)

    def pos_filter_step(self, v_uav, solved, key_rec, R_world, state=None, input=None, pos_filter=None, **settings):
        """ofk_pos_filter_step, the stage entry: rules 1-8 on host arrays.  v_uav [B,3], solved [B] of the step's record; key_rec
        [B,32] the keyframe's record of the step; R_world [B,3,3]; state: dict(x [B,12], P [B,12,12], istate [B,16] i32) of the
        previous call (None: not started, at zero); input [B,12] (None: none); the setting a PosFilter or pos_filter_setting's
        keywords.  -> (state, rec [B,48]), new arrays.  Touches no resident state."""
        f = pos_filter if pos_filter is not None else pos_filter_setting(**settings)
        vu = _arr(v_uav, np.float64)
        if vu.ndim != 2 or vu.shape[1] != 3 or vu.shape[0] < 1:
            raise ValueError(f"pos_filter_step: v_uav {vu.shape} is not [B >= 1, 3]")
        B = vu.shape[0]
        so = _arr(solved, np.int32, (B,)); kr = _arr(key_rec, np.float64, (B, KEY_DOUBLES)); rw = _arr(R_world, np.float64, (B, 3, 3))
        state = state or {}
        x = np.zeros((B, POSF_STATES), np.float64) if state.get("x") is None else np.array(_arr(state["x"], np.float64, (B, POSF_STATES)))
        P = np.zeros((B, POSF_STATES, POSF_STATES), np.float64) if state.get("P") is None \
            else np.array(_arr(state["P"], np.float64, (B, POSF_STATES, POSF_STATES)))
        ist = np.zeros((B, POSF_INTS), np.int32) if state.get("istate") is None else np.array(_arr(state["istate"], np.int32, (B, POSF_INTS)))
        inp = _opt(input, np.float64, (B, POSF_INPUT))
        rec = np.zeros((B, POSF_DOUBLES), np.float64)
        with self._lock:
            self._ck(self._L.ofk_pos_filter_step(self._h, C.byref(f), _p(vu), _p(so), _p(kr), _p(rw), _p(inp), _p(x), _p(P), _p(ist), B, _p(rec)))
        return dict(x=x, P=P, istate=ist), rec

    def zones_reset(self, batch=None):
        """ofk_zones_reset: the zone tables of the first `batch` streams (all by default) are cleared."""
        with self._lock:
            self._ck(self._L.ofk_zones_reset(self._h, int(self.max_batch if batch is None else batch)))

    def zones_download(self, batch=None):
        """ofk_zones_download -> dict(zones [batch,16,67] i32: ttl (0 = free), vertices, members, 32 x (x, y); motion [batch,16,4] f32:
        off x, y, flow x, y; stats [batch,8] i32 of the latest step: live, inserted, refreshed, evicted, rejects, absorbed, label
        sweeps, a reserved 0).  The library writes all max_batch streams; the first `batch` are returned."""
        zn, mo, st = self._rows("zones_download", self.max_batch if batch is None else int(batch),
                                lambda *p: self._L.ofk_zones_download(self._h, *p),
                                ((ZONE_MAX, ZONE_INTS), np.int32), ((ZONE_MAX, ZONE_FLOATS), np.float32), ((ZONE_STATS,), np.int32))
        return dict(zones=zn, motion=mo, stats=st)

    def zones_step(self, old_pts, new_pts, status, keep, counts, h, w, mask=None):
        """ofk_zones_step, the stage entry: one step of the zone rules on host arrays (old_pts / new_pts [B,S,2] f32, status / keep
        [B,S] u8, counts [B]) against the resident table -> the re-detection mask [B,h,w] u8 (mask, or all ones, with the zones zeroed)."""
        op = _arr(old_pts, np.float32)
        if op.ndim != 3 or op.shape[2] != 2 or op.shape[1] < 1:
            raise ValueError(f"zones_step: old_pts {op.shape} is not [B, S >= 1, 2]")
        B, S, _ = op.shape
        nw = _arr(new_pts, np.float32)
        if nw.shape != op.shape:
            raise ValueError(f"zones_step: new_pts {nw.shape} does not match old_pts {op.shape}")
        st = _arr(status, np.uint8, (B, S)); kp = _arr(keep, np.uint8, (B, S)); counts = _arr(counts, np.int32, (B,))
        h, w = int(h), int(w)
        mi = _opt(mask, np.uint8, (B, h, w))
        out = np.zeros((B, h, w), np.uint8)
        with self._lock:
            self._ck(self._L.ofk_zones_step(self._h, _p(op), _p(nw), _p(st), _p(kp), _p(counts), B, S, h, w, _p(mi), _p(out)))
        return out

    def set_camera(self, camera=None, **settings):
        """ofk_set_camera: a Camera (or camera_setting's keywords); None or model "off" switches it off.  Every later pairs_run and
        stream step hands its solve stage the ideal pixels of the tracked points; everything in the image keeps the raw ones.  The
        caller keeps the sensors' scaling, cx, cy at 1 / fo_x, co_x, co_y."""
        self._set_struct(self._L.ofk_set_camera, camera, settings, camera_setting, lock=True)

    def get_camera(self):
        return self._get_struct(self._L.ofk_get_camera, Camera)

    def _camera_points(self, fn, camera, pts, counts, out):
        single, (pp,), counts, _, (res,) = _point_arrays([pts], counts, None, [out], lambda shape: f"{fn}: pts {shape} is not [B, S, 2]")
        B, S = pp.shape[:2]
        if S > 0:
            with self._lock:
                self._ck(getattr(self._L, fn)(self._h, C.byref(camera), _p(pp), _p(counts), B, S, _p(res)))
        return res[0] if single else res

    def undistort_points(self, camera, pts, counts=None, out=None):
        """ofk_undistort_points: image pixels pts [B,S,2] (or [S,2]) f32 -> ideal pixels under `camera` (a Camera; fo_x != fo_y is
        accepted here); counts None = every point; entries beyond counts[b] keep what `out` holds (zeros without it)."""
        return self._camera_points("ofk_undistort_points", camera, pts, counts, out)

    def distort_points(self, camera, pts, counts=None, out=None):
        """ofk_distort_points: the forward map, ideal pixels -> image pixels; arguments as undistort_points."""
        return self._camera_points("ofk_distort_points", camera, pts, counts, out)

    def camera_download(self, batch):
        """ofk_camera_download: (prev_ideal, next_ideal) [batch,max_pts,2] f32, the ideal points the solve stage of the latest run or
        step with the camera on saw.  The library writes that run's rows, so the buffers have max_batch of them."""
        return self._points_download("ofk_camera_download", batch)

    def set_rolling_shutter(self, rshutter=None, **settings):
        """ofk_set_rolling_shutter: an RShutter (or rshutter_setting's keywords); None or mode "off" switches it off.  Every later
        pairs_run and stream step hands its solve stage the positions a global shutter would have seen at the two time stamps;
        everything in the image keeps the raw pixels."""
        self._set_struct(self._L.ofk_set_rolling_shutter, rshutter, settings, rshutter_setting, lock=True)

    def get_rolling_shutter(self):
        return self._get_struct(self._L.ofk_get_rolling_shutter, RShutter)

    def rs_correct_points(self, rshutter, raw_prev, raw_next, counts=None, sensors=None, ideal_prev=None, ideal_next=None, out=None):
        """ofk_rs_correct_points: raw_prev, raw_next [B,S,2] (or [S,2]) f32 image pixels of the tracked points (their rows give the
        capture times), ideal_prev / ideal_next the ideal pixels of the same points (both None: the raw ones) -> (prev, next) as a
        global shutter would have seen them at the two time stamps.  rshutter: an RShutter with rows > 0; sensors [B,28] (needed in
        gyro mode); counts None = every point; entries beyond counts[b] keep what out = (prev, next) holds (zeros without it)."""
        single, (rp, rn), counts, sn, (o0, o1) = _point_arrays(
            [raw_prev, raw_next], counts, sensors, [None, None] if out is None else [out[0], out[1]],
            lambda a, b: f"rs_correct_points: points {a} / {b} are not two [B, S, 2] arrays")
        B, S = rp.shape[:2]
        if (ideal_prev is None) != (ideal_next is None):
            raise ValueError("rs_correct_points: ideal_prev and ideal_next come together")
        ip = None if ideal_prev is None else _arr(ideal_prev, np.float32).reshape(rp.shape)
        inx = None if ideal_next is None else _arr(ideal_next, np.float32).reshape(rp.shape)
        if S > 0:
            with self._lock:
                self._ck(self._L.ofk_rs_correct_points(self._h, C.byref(rshutter), _p(rp), _p(rn), _p(ip), _p(inx), _p(counts), B, S, _p(sn), _p(o0), _p(o1)))
        return (o0[0], o1[0]) if single else (o0, o1)

    def rs_download(self, batch):
        """ofk_rs_download: (prev, next) [batch,max_pts,2] f32, the points the solve stage of the latest run or step with the rolling
        shutter on saw.  The library writes that run's rows, so the buffers have max_batch of them."""
        return self._points_download("ofk_rs_download", batch)

    def set_finite_motion(self, finite_motion=None, **settings):
        """ofk_set_finite_motion: a FiniteMotion (or finite_motion_setting's keywords); None or mode "off" switches it off.  Every
        later pairs_run and stream step hands its solve stage the points for which the first-order system is the exact relation of
        the frame pair; the velocity is then the displacement per frame interval.  Everything in the image keeps the raw pixels."""
        self._set_struct(self._L.ofk_set_finite_motion, finite_motion, settings, finite_motion_setting, lock=True)

    def get_finite_motion(self):
        return self._get_struct(self._L.ofk_get_finite_motion, FiniteMotion)

    def finite_correct_points(self, finite_motion, prev, next, counts=None, sensors=None, out=None):
        """ofk_finite_correct_points: prev, next [B,S,2] (or [S,2]) f32, the points the solve would otherwise read -> (prev, next)
        rewritten for the finite motion of sensors [B,28] (normal, omega, scaling, centre).  counts None = every point; entries
        beyond counts[b] keep what out = (prev, next) holds (zeros without it)."""
        single, (pp, pn), counts, sn, (o0, o1) = _point_arrays(
            [prev, next], counts, sensors, [None, None] if out is None else [out[0], out[1]],
            lambda a, b: f"finite_correct_points: points {a} / {b} are not two [B, S, 2] arrays")
        B, S = pp.shape[:2]
        if S > 0:
            with self._lock:
                self._ck(self._L.ofk_finite_correct_points(self._h, C.byref(finite_motion), _p(pp), _p(pn), _p(counts), B, S, _p(sn), _p(o0), _p(o1)))
        return (o0[0], o1[0]) if single else (o0, o1)

    def finite_download(self, batch):
        """ofk_finite_download: (prev, next) [batch,max_pts,2] f32, the points the solve stage of the latest run or step with the
        finite motion on saw.  The library writes that run's rows, so the buffers have max_batch of them."""
        return self._points_download("ofk_finite_download", batch)

    def track_gate_download(self, batch, points=True):
        """ofk_track_gate_download of the latest gated run / step -> dict(stats [batch,4] i32: forward-tracked, of those lost by the
        backward pass, of the rest beyond fb_thr, of the rest over err_max; and, with points, fb2 [batch,max_pts] f32, back_pts
        [batch,max_pts,2] f32, back_status [batch,max_pts] u8 - zeros when only the err cap was on).  The library writes the rows of
        the latest run, whatever `batch` says, so the buffers have max_batch rows and the first `batch` are returned."""
        S = self.max_pts
        per_point = [((S,), np.float32), ((S, 2), np.float32), ((S,), np.uint8)] if points else []
        st, *pts = self._rows("track_gate_download", batch, lambda st, *p: self._L.ofk_track_gate_download(self._h, *(p or [None] * 3), S, st),
                              ((4,), np.int32), *per_point)
        return dict(stats=st, **dict(zip(("fb2", "back_pts", "back_status"), pts)))

    def track_gate_stats(self, batch):
        """The four counts per image of the latest gated run / step alone ([batch,4] int32): no per-point array is copied."""
        return self.track_gate_download(batch, points=False)["stats"]

    def lk_pyr_fb(self, prev, nxt, prev_pts, counts, gate=None, win=15, max_level=3, max_count=20, eps=0.03, min_eig_thr=1e-4,
                  next_pts=None, flags=0, light=None, **settings):
        """ofk_lk_pyr_fb: the batched lk_pyr (prev, nxt [B,h,w]; prev_pts [B,S,2]; counts [B]) with the track gates behind it.
        gate: a TrackGate, or track_gate_setting's keywords.  -> dict(next_pts, status (gated), err, back_pts, back_status, fb2).
        light: None, "bias", "gain" or an LkLight - both passes under ofk_lk_light, ofk_lk_pyr_light (only when given and on)."""
        g = gate if gate is not None else track_gate_setting(**settings)
        light = _light(light)
        flags = int(flags)
        if flags & LK_USE_INITIAL_FLOW and next_pts is None:
            raise ValueError("lk_pyr_fb: LK_USE_INITIAL_FLOW needs next_pts")
        prev = _arr(prev, np.uint8); nxt = _arr(nxt, np.uint8)
        if prev.ndim != 3 or nxt.shape != prev.shape:
            raise ValueError(f"lk_pyr_fb: frames {prev.shape} / {nxt.shape} are not two [B, h, w] batches of one shape")
        B, h, w = prev.shape
        pp = _arr(prev_pts, np.float32)
        if pp.ndim != 3 or pp.shape[0] != B or pp.shape[2] != 2 or pp.shape[1] < 1:
            raise ValueError(f"lk_pyr_fb: prev_pts {pp.shape} is not [{B}, S >= 1, 2]")
        S = pp.shape[1]
        counts = _arr(counts, np.int32, (B,))
        init = None
        if flags & LK_USE_INITIAL_FLOW:
            init = _arr(next_pts, np.float32)
            if init.shape != pp.shape:
                raise ValueError(f"lk_pyr_fb: next_pts {init.shape} does not match prev_pts {pp.shape}")
        out = dict(next_pts=np.zeros((B, S, 2), np.float32), status=np.zeros((B, S), np.uint8), err=np.zeros((B, S), np.float32),
                   back_pts=np.zeros((B, S, 2), np.float32), back_status=np.zeros((B, S), np.uint8), fb2=np.zeros((B, S), np.float32))
        args = (self._h, _p(prev), _p(nxt), B, h, w, _p(pp), _p(counts), S, int(win), int(max_level), int(max_count), float(eps),
                float(min_eig_thr), _p(init), flags, _p(out["next_pts"]), _p(out["status"]), _p(out["err"]), C.byref(g), _p(out["back_pts"]),
                _p(out["back_status"]), _p(out["fb2"]))
        with self._lock:
            self._ck(self._L.ofk_lk_pyr_fb(*args) if light is None else self._L.ofk_lk_pyr_light(*args, C.byref(light)))
        return out

    # ------------------------------------------------------------------ estimation
    def flow_model(self, x, v, omega, d, nrm, t=None):
        x = _arr(x, np.float64)
        if x.ndim not in (2, 3) or x.shape[-1] != 2:
            raise ValueError(f"flow_model: x {x.shape} must be [..., n, 2]")
        single = x.ndim == 2
        if single:
            x = x[None]
        B, n, _ = x.shape
        v = _arr(v, np.float64, (B, 3)); omega = _arr(omega, np.float64, (B, 3)); nrm = _arr(nrm, np.float64, (B, 3))
        d = _arr(d, np.float64, (B,)); t = _opt(t, np.float64, (B, 3))
        out = np.empty((B, n, 2), np.float64)
        if n:
            with self._lock:
                self._ck(self._L.ofk_flow_model(self._h, _p(x), B, n, _p(v), _p(omega), _p(d), _p(nrm), _p(t), _p(out)))
        return out[0] if single else out

    def feasibility(self, variant, x, u, nrm, v, dist=None, omega=None, t=None):
        x = _arr(x, np.float64); u = _arr(u, np.float64)
        if u.shape != x.shape or x.shape[-1] != 2:
            raise ValueError(f"feasibility: x {x.shape} and u {u.shape} must both be [..., n, 2]")
        single = x.ndim == 2
        if single:
            x = x[None]; u = u[None]
        B, n, _ = x.shape
        nrm = _arr(nrm, np.float64, (B, 3)); v = _arr(v, np.float64, (B, 3))
        dist = _opt(dist, np.float64, (B,)); omega = _opt(omega, np.float64, (B, 3)); t = _opt(t, np.float64, (B, 3))
        r = np.empty((B, n), np.float64); dd = np.empty((B, n), np.float64)
        if n:
            with self._lock:
                self._ck(self._L.ofk_feasibility(self._h, int(variant), _p(x), _p(u), B, n, _p(nrm), _p(v), _p(dist), _p(omega),
                                                 _p(t), _p(r), _p(dd)))
        return (r[0], dd[0]) if single else (r, dd)

    def velocity_solve(self, variant, x, u, d=None, nrm=None, omega=None, t=None, wgt=None, valid=None):
        """Returns out [B,8] = v[3], residual SS, rank, s[3] (single problem: [8])."""
        x = _arr(x, np.float64); u = _arr(u, np.float64)
        if u.shape[:-1] != x.shape[:-1] or x.shape[-1] != 2 or u.shape[-1] < 2:
            raise ValueError(f"velocity_solve: x {x.shape} must be [..., n, 2] and u {u.shape} [..., n, >=2] over the same points")
        single = x.ndim == 2
        if single:
            x = x[None]; u = u[None]
        B, n, _ = x.shape
        u = _arr(u[..., :2], np.float64)
        nrm = _arr(nrm, np.float64, (B, 3))
        d = _opt(d, np.float64, (B,)); omega = _opt(omega, np.float64, (B, 3)); t = _opt(t, np.float64, (B, 3))
        wgt = _opt(wgt, np.float64, (B, n)); valid = _opt(valid, np.uint8, (B, n))
        out = np.zeros((B, SOLVE_DOUBLES), np.float64)
        if n:
            with self._lock:
                self._ck(self._L.ofk_velocity_solve(self._h, int(variant), _p(x), _p(u), _p(valid), B, n, _p(d), _p(nrm),
                                                    _p(omega), _p(t), _p(wgt), _p(out)))
        return out[0] if single else out

    def velocity_solve_robust(self, variant, x, u, d=None, nrm=None, omega=None, t=None, wgt=None, valid=None, robust=None, **settings):
        """ofk_velocity_solve_robust: velocity_solve's arguments plus the setting (a Robust, or robust_setting's keywords).
        Returns out [B,8], weights [B,n], stats [B,8] (single problem: [8], [n], [8])."""
        r = robust if robust is not None else robust_setting(**settings)
        x = _arr(x, np.float64); u = _arr(u, np.float64)
        if u.shape[:-1] != x.shape[:-1] or x.shape[-1] != 2 or u.shape[-1] < 2:
            raise ValueError(f"velocity_solve_robust: x {x.shape} must be [..., n, 2] and u {u.shape} [..., n, >=2] over the same points")
        single = x.ndim == 2
        if single:
            x = x[None]; u = u[None]
        B, n, _ = x.shape
        u = _arr(u[..., :2], np.float64)
        nrm = _arr(nrm, np.float64, (B, 3))
        d = _opt(d, np.float64, (B,)); omega = _opt(omega, np.float64, (B, 3)); t = _opt(t, np.float64, (B, 3))
        wgt = _opt(wgt, np.float64, (B, n)); valid = _opt(valid, np.uint8, (B, n))
        out = np.zeros((B, SOLVE_DOUBLES), np.float64); w = np.zeros((B, n), np.float64); st = np.zeros((B, ROBUST_DOUBLES), np.float64)
        if not n:                                               # no points: velocity_solve's zeros, flag 1
            st[:, 4] = -1.0; st[:, 7] = 1.0
            return (out[0], w[0], st[0]) if single else (out, w, st)
        with self._lock:
            self._ck(self._L.ofk_velocity_solve_robust(self._h, int(variant), _p(x), _p(u), _p(valid), B, n, _p(d), _p(nrm), _p(omega),
                                                       _p(t), _p(wgt), C.byref(r), _p(out), _p(w), _p(st)))
        return (out[0], w[0], st[0]) if single else (out, w, st)

    def set_robust(self, robust=None, **settings):
        """ofk_set_robust: a Robust (or robust_setting's keywords); None or loss "off" switches it off.  Every later pairs_run and
        stream step solves robustly."""
        self._set_struct(self._L.ofk_set_robust, robust, settings, robust_setting, lock=False)

    def get_robust(self):
        return self._get_struct(self._L.ofk_get_robust, Robust)

    def robust_download(self, batch):
        """(weights [batch, max_pts], stats [batch, 8]) of the latest run / step with the setting on."""
        return tuple(self._rows(None, batch, lambda w, st: self._L.ofk_robust_download(self._h, w, self.max_pts, st),
                                ((self.max_pts,), np.float64), ((ROBUST_DOUBLES,), np.float64)))

    def _velocity_solve_second(self, name, variant, x, u, d, nrm, omega, t, valid, robust, setting, doubles, no_points, points=False):
        """ofk_velocity_solve_<name>: the marshalling the second-stage stage entries share.  no_points(rec, d, nrm, omega) fills the
        records of a call without points.  Returns (out, rec) or, with points, (out, rec, point rows)."""
        x = _arr(x, np.float64); u = _arr(u, np.float64)
        if u.shape[:-1] != x.shape[:-1] or x.shape[-1] != 2 or u.shape[-1] < 2:
            raise ValueError(f"velocity_solve_{name}: x {x.shape} must be [..., n, 2] and u {u.shape} [..., n, >=2] over the same points")
        single = x.ndim == 2
        if single:
            x = x[None]; u = u[None]
        B, n, _ = x.shape
        u = _arr(u[..., :2], np.float64)
        nrm = _arr(nrm, np.float64, (B, 3))
        d = _opt(d, np.float64, (B,)); omega = _opt(omega, np.float64, (B, 3)); t = _opt(t, np.float64, (B, 3))
        valid = _opt(valid, np.uint8, (B, n))
        res = [np.zeros((B, SOLVE_DOUBLES), np.float64), np.zeros((B, doubles), np.float64)] + ([np.zeros((B, n, 4), np.float64)] if points else [])
        if not n:                                               # no points: velocity_solve's zeros
            no_points(res[1], d, nrm, omega)
        else:
            with self._lock:
                self._ck(getattr(self._L, "ofk_velocity_solve_" + name)(
                    self._h, int(variant), _p(x), _p(u), _p(valid), B, n, _p(d), _p(nrm), _p(omega), _p(t), None,
                    C.byref(robust) if robust is not None else None, C.byref(setting), *[_p(a) for a in res]))
        return tuple(a[0] for a in res) if single else tuple(res)

    def _records_download(self, name, batch, *shape):
        """ofk_<name>_download into [max_batch, *shape]: its first `batch` rows."""
        return self._rows(None, batch, lambda rec: getattr(self._L, f"ofk_{name}_download")(self._h, rec), (shape, np.float64))[0]

    def velocity_solve_cov(self, variant, x, u, d=None, nrm=None, omega=None, t=None, valid=None, robust=None, cov=None, **settings):
        """ofk_velocity_solve_cov: velocity_solve's arguments (NODE or SIM), an optional Robust and the covariance setting (a Cov, or
        cov_setting's keywords).  Returns out [B,8], cov [B,24] (single problem: [8], [24])."""
        cv = cov if cov is not None else cov_setting(**settings)
        def void(rec, d, nrm, omega):                           # a void covariance
            rec[:, 13] = 1.0
        return self._velocity_solve_second("cov", variant, x, u, d, nrm, omega, t, valid, robust, cv, COV_DOUBLES, void)

    def set_cov(self, cov=None, **settings):
        """ofk_set_cov: a Cov (or cov_setting's keywords); None or mode "off" switches it off.  Every later pairs_run, pairs filter step
        and stream step computes the covariance records (and, with filter_r / nis_max, corrects its filter with them)."""
        self._set_struct(self._L.ofk_set_cov, cov, settings, cov_setting, lock=False)

    def get_cov(self):
        return self._get_struct(self._L.ofk_get_cov, Cov)

    def cov_download(self, batch):
        """cov [batch, 24] of the latest run / step with the setting on."""
        return self._records_download("cov", batch, COV_DOUBLES)

    def velocity_solve_joint(self, variant, x, u, d=None, nrm=None, omega=None, t=None, valid=None, robust=None, joint=None, **settings):
        """ofk_velocity_solve_joint: velocity_solve's arguments (NODE or SIM), an optional Robust and the joint setting (a Joint, or
        joint_setting's keywords).  Returns out [B,8] after the joint rewrite, joint [B,32] (single problem: [8], [32])."""
        jv = joint if joint is not None else joint_setting(**settings)
        def nothing(rec, d, nrm, omega):                        # nothing attempted
            if omega is not None:
                rec[:, 0:3] = omega
            rec[:, 10] = 1.0
        return self._velocity_solve_second("joint", variant, x, u, d, nrm, omega, t, valid, robust, jv, JOINT_DOUBLES, nothing)

    def set_joint(self, joint=None, **settings):
        """ofk_set_joint: a Joint (or joint_setting's keywords); None or mode False switches it off.  Every later pairs_run and stream
        step refines the gyro from the flow and rewrites v, the residual and v_uav of its records."""
        self._set_struct(self._L.ofk_set_joint, joint, settings, joint_setting, lock=False)

    def get_joint(self):
        return self._get_struct(self._L.ofk_get_joint, Joint)

    def joint_download(self, batch):
        """joint [batch, 32] of the latest run / step with the setting on."""
        return self._records_download("joint", batch, JOINT_DOUBLES)

    def set_gyro_bias(self, gyro_bias=None, **settings):
        """ofk_set_gyro_bias: a GyroBias (or gyro_bias_setting's keywords); None or mode False switches it off.  Every later stream step
        takes the stream's bias out of omega in front of everything and, with update on, filters it from the flow."""
        self._set_struct(self._L.ofk_set_gyro_bias, gyro_bias, settings, gyro_bias_setting, lock=False)

    def get_gyro_bias(self):
        return self._get_struct(self._L.ofk_get_gyro_bias, GyroBias)

    def gyro_bias_reset(self, state):
        """ofk_gyro_bias_reset: state [batch, 9] = b (3), P upper triangle (6), loaded into the first `batch` streams."""
        state = _arr(np.atleast_2d(np.asarray(state, np.float64)), np.float64)
        if state.ndim != 2 or state.shape[1] != 9:
            raise ValueError(f"gyro_bias_reset: state {state.shape} must be [batch, 9]")
        with self._lock:
            self._ck(self._L.ofk_gyro_bias_reset(self._h, _p(state), state.shape[0]))

    def gyro_bias_download(self, batch):
        """bias [batch, 32] of the latest stream step with the setting on."""
        return self._records_download("gyro_bias", batch, BIAS_DOUBLES)

    def gyro_bias_step(self, variant, x, u, d=None, nrm=None, omega=None, state=None, valid=None, robust=None, gyro_bias=None, **settings):
        """ofk_gyro_bias_step: velocity_solve's arguments (NODE or SIM; omega the raw gyro), an optional Robust, the setting (a GyroBias, or
        gyro_bias_setting's keywords) and state [B,32] (None: the setting's own start).  Returns out [B,8], state [B,32] after the step
        (single problem: [8], [32])."""
        gv = gyro_bias if gyro_bias is not None else gyro_bias_setting(**settings)
        x = _arr(x, np.float64); u = _arr(u, np.float64)
        if u.shape[:-1] != x.shape[:-1] or x.shape[-1] != 2 or u.shape[-1] < 2:
            raise ValueError(f"gyro_bias_step: x {x.shape} must be [..., n, 2] and u {u.shape} [..., n, >=2] over the same points")
        single = x.ndim == 2
        if single:
            x = x[None]; u = u[None]
        B, n, _ = x.shape
        if not n:
            raise ValueError("gyro_bias_step: no points")
        u = _arr(u[..., :2], np.float64)
        nrm = _arr(nrm, np.float64, (B, 3))
        d = _opt(d, np.float64, (B,)); omega = _opt(omega, np.float64, (B, 3)); valid = _opt(valid, np.uint8, (B, n))
        if state is None:
            st = np.zeros((B, BIAS_DOUBLES), np.float64)
            st[:, 0:3] = list(gv.b0); st[:, [3, 6, 8]] = np.asarray(list(gv.p0)) ** 2
        else:
            st = _arr(np.array(state, np.float64), np.float64, (B, BIAS_DOUBLES))
        out = np.zeros((B, SOLVE_DOUBLES), np.float64)
        with self._lock:
            self._ck(self._L.ofk_gyro_bias_step(self._h, int(variant), _p(x), _p(u), _p(valid), B, n, _p(d), _p(nrm), _p(omega), None,
                                                C.byref(robust) if robust is not None else None, C.byref(gv), _p(st), _p(out)))
        return (out[0], st[0]) if single else (out, st)

    def velocity_solve_plane(self, variant, x, u, d=None, nrm=None, omega=None, t=None, valid=None, robust=None, plane=None, **settings):
        """ofk_velocity_solve_plane: velocity_solve's arguments (NODE or SIM), an optional Robust and the plane setting (a Plane, or
        plane_setting's keywords).  Returns out [B,8] after the rewrite, plane [B,32] (single problem: [8], [32])."""
        pv = plane if plane is not None else plane_setting(**settings)
        def nothing(rec, d, nrm, omega):                        # nothing attempted
            rec[:, 0:3] = nrm
            if d is not None:
                rec[:, 3] = d
            rec[:, 10] = 1.0
        return self._velocity_solve_second("plane", variant, x, u, d, nrm, omega, t, valid, robust, pv, PLANE_DOUBLES, nothing)

    def set_plane(self, plane=None, **settings):
        """ofk_set_plane: a Plane (or plane_setting's keywords); None or mode False switches it off.  Every later pairs_run and stream
        step refines the ground normal from the flow and rewrites v, the residual and v_uav of its records."""
        self._set_struct(self._L.ofk_set_plane, plane, settings, plane_setting, lock=False)

    def get_plane(self):
        return self._get_struct(self._L.ofk_get_plane, Plane)

    def plane_download(self, batch):
        """plane [batch, 32] of the latest run / step with the setting on."""
        return self._records_download("plane", batch, PLANE_DOUBLES)

    def velocity_solve_epipolar(self, variant, x, u, d=None, nrm=None, omega=None, t=None, valid=None, robust=None, epipolar=None, **settings):
        """ofk_velocity_solve_epipolar: velocity_solve's arguments (NODE or SIM), an optional Robust and the epipolar setting (an
        Epipolar, or epipolar_setting's keywords).  Returns out [B,8] after the rewrite, the record [B,32] and the point rows
        [B,n,4] (single problem: [8], [32], [n,4])."""
        ev = epipolar if epipolar is not None else epipolar_setting(**settings)
        def nothing(rec, d, nrm, omega):                        # nothing attempted
            rec[:, 10] = 1.0
        return self._velocity_solve_second("epipolar", variant, x, u, d, nrm, omega, t, valid, robust, ev, EPI_DOUBLES, nothing, points=True)

    def set_epipolar(self, epipolar=None, **settings):
        """ofk_set_epipolar: an Epipolar (or epipolar_setting's keywords); None or mode False switches it off.  Every later pairs_run
        and stream step takes v from the epipolar constraint and the range at the beam's foot, and rewrites v, field 3 and v_uav of
        its records."""
        self._set_struct(self._L.ofk_set_epipolar, epipolar, settings, epipolar_setting, lock=False)

    def get_epipolar(self):
        return self._get_struct(self._L.ofk_get_epipolar, Epipolar)

    def epipolar_download(self, batch):
        """The record [batch, 32] and the point rows [batch, max_pts, 4] (rho, r, |b|, flag) of the latest run / step with the
        setting on."""
        with self._lock:                                         # both from the same run
            return self._records_download("epipolar", batch, EPI_DOUBLES), self._records_download("epipolar_points", batch, self.max_pts, 4)

    def imu_propagate(self, state, msg):
        state = _arr(state, np.float64).copy(); msg = _arr(msg, np.float64)
        single = state.ndim == 1
        s2 = state.reshape(-1, IMU_STATE); m2 = msg.reshape(-1, IMU_MSG)
        with self._lock:
            self._ck(self._L.ofk_imu_propagate(self._h, _p(s2), _p(m2), len(s2)))
        return s2[0] if single else s2

    def post_solve(self, v_obs, rotation, ang, offset):
        v_obs = _arr(v_obs, np.float64)
        single = v_obs.ndim == 1
        v2 = v_obs.reshape(-1, 3); B = len(v2)
        R = _arr(np.asarray(rotation, np.float64).reshape(-1, 9), np.float64, (B, 9))
        ang = _arr(ang, np.float64, (B, 3)); offset = _arr(offset, np.float64, (B, 3))
        out = np.empty((B, 3), np.float64)
        with self._lock:
            self._ck(self._L.ofk_post_solve(self._h, _p(v2), _p(R), _p(ang), _p(offset), B, _p(out)))
        return out[0] if single else out

    def feature_eval(self, pos, pos_err, oldpos, oldpos_err, vel, vel_err, focal_len, dummy_value, img_dim, weight, counts=None):
        """calc_height + dynamic_immobile + eval_ft of of_library.py for a batch of track sets ([batch, n, 2] positions;
        a single [n, 2] set is accepted).  Returns dict(height, height_err, immobile, score, order, bad_height)."""
        pos = _arr(pos, np.float64)
        single = pos.ndim == 2
        pos = pos.reshape((1,) + pos.shape) if single else pos
        B, n = pos.shape[0], pos.shape[1]
        def per_feature(a):                                      # scalar, [n] or [B, n]
            a = np.asarray(a, np.float64)
            return _arr(np.broadcast_to(a if a.size == 1 else a.reshape(-1, n), (B, n)), np.float64)
        pos_err = per_feature(pos_err)
        oldpos = _arr(np.asarray(oldpos, np.float64).reshape(B, n, 2), np.float64)
        oldpos_err = per_feature(oldpos_err)
        vel = _arr(np.broadcast_to(np.asarray(vel, np.float64).reshape(-1, 3), (B, 3)), np.float64)
        vel_err = _arr(np.broadcast_to(np.asarray(vel_err, np.float64).reshape(-1, 3), (B, 3)), np.float64)
        cn = np.full(B, n, np.int32) if counts is None else _arr(counts, np.int32, (B,))
        w = _arr(weight, np.float64, (4,))
        out = dict(height=np.zeros((B, n)), height_err=np.zeros((B, n)), immobile=np.zeros((B, n), np.uint8), score=np.zeros((B, n)),
                   order=np.zeros((B, n), np.int32))
        bad = C.c_int(0)
        with self._lock:
            self._ck(self._L.ofk_feature_eval(self._h, _p(pos), _p(pos_err), _p(oldpos), _p(oldpos_err), _p(cn), B, n, _p(vel), _p(vel_err),
                                              float(focal_len), float(dummy_value), int(img_dim[0]), int(img_dim[1]), _p(w),
                                              _p(out["height"]), _p(out["height_err"]), _p(out["immobile"]), _p(out["score"]),
                                              _p(out["order"]), C.byref(bad)))
        out["bad_height"] = bool(bad.value)
        if single:
            out = {k: (v[0] if isinstance(v, np.ndarray) else v) for k, v in out.items()}
        return out

    def d_split(self, d, d_exp_err, counts=None):
        """node:249-252: sorted plane distances, their consecutive differences and the number of gaps >= d_exp_err, per set
        ([batch, n] or a single [n])."""
        d = _arr(d, np.float64)
        single = d.ndim == 1
        d = d.reshape(1, -1) if single else d
        B, n = d.shape
        cn = np.full(B, n, np.int32) if counts is None else _arr(counts, np.int32, (B,))
        srt = np.zeros((B, n)); dif = np.zeros((B, n)); ns = np.zeros(B, np.int32)
        with self._lock:
            self._ck(self._L.ofk_d_split(self._h, _p(d), _p(cn), B, n, float(d_exp_err), _p(srt), _p(dif), _p(ns)))
        return (srt[0], dif[0, :max(n - 1, 0)], int(ns[0])) if single else (srt, dif, ns)

    def associate_sensors(self, t_img, imu_t, imu_quat, imu_omega, hgt_t, hgt_range, sensors=None):
        """evaluate_exp.py:68-95 on the device: nearest IMU / range sample per image time -> (sensors, imu_index, hgt_index).
        `sensors` ([n_img, 28]) supplies the fields the association does not touch (offset, scaling, centre, prior)."""
        t_img = _arr(np.atleast_1d(t_img), np.float64); n = len(t_img)
        imu_t = _arr(imu_t, np.float64); ni = len(imu_t)
        q = _arr(imu_quat, np.float64, (ni, 4)); w = _arr(imu_omega, np.float64, (ni, 3))
        hgt_t = _arr(hgt_t, np.float64); nh = len(hgt_t); r = _arr(hgt_range, np.float64, (nh,))
        out = make_sensors(n) if sensors is None else np.array(_arr(sensors, np.float64, (n, SENSOR_DOUBLES)))
        ii = np.empty(n, np.int32); hi = np.empty(n, np.int32)
        with self._lock:
            self._ck(self._L.ofk_associate_sensors(self._h, _p(t_img), n, _p(imu_t), _p(q), _p(w), ni, _p(hgt_t), _p(r), nh,
                                                   _p(out), _p(ii), _p(hi)))
        return out, ii, hi

    def kf_predict_update(self, F, H, Q, R, x, P, B=None, u=None, z=None, do_predict=True):
        F = _arr(F, np.float64); H = _arr(H, np.float64); Q = _arr(Q, np.float64); R = _arr(R, np.float64)
        ns = F.shape[0]; nm = H.shape[0]
        x = _arr(x, np.float64).copy(); P = _arr(P, np.float64).copy()
        single = x.ndim == 1
        x2 = x.reshape(-1, ns); batch = len(x2); P2 = P.reshape(batch, ns, ns)
        nc = 0
        if B is not None and u is not None:
            B = _arr(B, np.float64); nc = B.shape[1]; u = _arr(u, np.float64, (batch, nc))
        else:
            B = None; u = None
        z = _opt(z, np.float64, (batch, nm))
        with self._lock:
            self._ck(self._L.ofk_kf_predict_update(self._h, ns, nm, nc, _p(F), _p(B), _p(H), _p(Q), _p(R), _p(x2), _p(P2), _p(u),
                                                   _p(z), batch, 1 if do_predict else 0))
        return (x2[0], P2[0]) if single else (x2, P2)

    def of_simulation(self, truth, sig, pos, true_flow, z):
        truth = _arr(truth, np.float64, (13,)); sig = _arr(sig, np.float64, (6,))
        pos = _arr(pos, np.float64); true_flow = _arr(true_flow, np.float64)
        n = len(pos)
        z = _arr(z, np.float64).reshape(-1, 10 + 4 * n)
        trials = len(z)
        v = np.empty((trials, 3), np.float64); bound = np.empty(trials, np.float64)
        with self._lock:
            self._ck(self._L.ofk_of_simulation(self._h, _p(truth), _p(sig), _p(pos), _p(true_flow), n, _p(z), trials, _p(v), _p(bound)))
        return v, bound

    def of_simulation_rng(self, truth, sig, pos, true_flow, seed, step, trials, trial0=0):
        """of_simulation with the normals drawn on the device (ofk_of_simulation_rng: Philox4x32-10 + Box-Muller keyed by (seed, step,
        global trial index)).  Returns (v_obs [trials, 3], bound [trials])."""
        truth = _arr(truth, np.float64, (13,)); sig = _arr(sig, np.float64, (6,))
        pos = _arr(pos, np.float64); true_flow = _arr(true_flow, np.float64)
        n = len(pos)
        v = np.empty((int(trials), 3), np.float64); bound = np.empty(int(trials), np.float64)
        with self._lock:
            self._ck(self._L.ofk_of_simulation_rng(self._h, _p(truth), _p(sig), _p(pos), _p(true_flow), n, C.c_ulonglong(int(seed)), C.c_uint(int(step)),
                                                   C.c_uint(int(trial0)), int(trials), _p(v), _p(bound)))
        return v, bound

    def noise_normals(self, seed, step, trial, count):
        """Elements 0 .. count - 1 of the device generator's row for (seed, step, trial)."""
        out = np.empty(int(count), np.float64)
        with self._lock:
            self._ck(self._L.ofk_noise_normals(self._h, C.c_ulonglong(int(seed)), C.c_uint(int(step)), C.c_uint(int(trial)), int(count), _p(out)))
        return out

    def feas_simulation(self, truth, sig, pos, true_flow, z, per_trial=False):
        """simulation.py:70-104 for all trials in one launch.  Returns (mean [6, n] in the reference's return order, v_obs
        [trials, 3]) and, with per_trial=True, the per-trial table [trials, 6, n] as a third item."""
        truth = _arr(truth, np.float64, (16,)); sig = _arr(sig, np.float64, (7,))
        pos = _arr(pos, np.float64); true_flow = _arr(true_flow, np.float64)
        n = len(pos)
        if pos.shape != (n, 2) or true_flow.shape != (n, 2):
            raise ValueError("feas_simulation: pos and true_flow must be [n, 2]")
        z = _arr(z, np.float64).reshape(-1, 12 + 4 * n)
        trials = len(z)
        mean = np.empty((6, n), np.float64); v = np.empty((trials, 3), np.float64)
        per = np.empty((trials, 6, n), np.float64) if per_trial else None
        with self._lock:
            self._ck(self._L.ofk_feas_simulation(self._h, _p(truth), _p(sig), _p(pos), _p(true_flow), n, _p(z), trials, _p(mean), _p(per), _p(v)))
        return (mean, v, per) if per_trial else (mean, v)

    def hist_overlap(self, data1, data2, bins=100):
        """overlap(data1, data2) of simulation.py:124-136."""
        d1 = _arr(np.ravel(data1), np.float64); d2 = _arr(np.ravel(data2), np.float64)
        out = C.c_int(0)
        with self._lock:
            self._ck(self._L.ofk_hist_overlap(self._h, _p(d1), len(d1), _p(d2), len(d2), int(bins), C.byref(out)))
        return int(out.value)

    # ------------------------------------------------------------------ resident frame-pair pipeline
    def pairs_upload(self, prev_bgr, next_bgr):
        prev_bgr, _ = self._batched(prev_bgr, 3); next_bgr, _ = self._batched(next_bgr, 3)
        prev_bgr = _arr(prev_bgr, np.uint8); next_bgr = _arr(next_bgr, np.uint8)
        B, h, w, ch = prev_bgr.shape
        if ch != 3 or next_bgr.shape != prev_bgr.shape:
            raise ValueError("expected two [B,h,w,3] BGR batches of equal shape")
        with self._lock:
            self._ck(self._L.ofk_pairs_upload(self._h, _p(prev_bgr), _p(next_bgr), B, h, w))
        self._resident = (B, h, w)

    @staticmethod
    def _jpeg_args(streams):
        bufs = [bytes(s) for s in streams]
        ptrs = (C.c_char_p * len(bufs))(*bufs)
        sizes = (C.c_size_t * len(bufs))(*[len(b) for b in bufs])
        return bufs, ptrs, sizes

    def pairs_upload_jpeg(self, prev_streams, next_streams):
        """Resident frame pairs from baseline JPEG streams (CompressedImage payloads), decoded on the device."""
        if len(prev_streams) != len(next_streams) or not len(prev_streams):
            raise ValueError("expected two equally long, non-empty lists of JPEG streams")
        h, w, _ = jpeg_info(prev_streams[0])
        keep0, p0, s0 = self._jpeg_args(prev_streams)
        keep1, p1, s1 = self._jpeg_args(next_streams)
        with self._lock:
            self._ck(self._L.ofk_pairs_upload_jpeg(self._h, p0, s0, p1, s1, len(keep0)))
        self._resident = (len(keep0), h, w)

    def jpeg_stage(self, slot, streams):
        """Phase 1 of the compressed ingest (ofk_jpeg_stage): parse + staging copy + asynchronous H2D of `streams` into staging slot
        0 / 1.  Takes no context lock: it is meant to run on a helper thread while the owner thread decodes the other slot.
        Returns (count, h, w)."""
        if not len(streams):
            raise ValueError("no streams")
        h, w, _ = jpeg_info(streams[0])
        keep, ptrs, sizes = self._jpeg_args(streams)
        rc = self._L.ofk_jpeg_stage(self._h, int(slot), ptrs, sizes, len(keep))
        if rc != OK:                                             # the slot's own message: the owner thread may be writing the context's
            raise OfkError(rc, self._L.ofk_jpeg_stage_error(self._h, int(slot)).decode())
        return len(keep), h, w

    def pairs_upload_staged(self, slot, staged):
        """Phase 2 (ofk_pairs_upload_staged): decodes the 2 B streams staged in `slot` (B previous frames, then B next frames) into
        the resident pair buffers.  `staged` = what jpeg_stage returned for that slot."""
        count, h, w = staged
        with self._lock:
            self._ck(self._L.ofk_pairs_upload_staged(self._h, int(slot)))
        self._resident = (count // 2, h, w)

    def jpeg_decode(self, streams):
        """[B,h,w,3] BGR uint8 from B baseline JPEG streams of one size and sampling (cv2.imdecode, batched)."""
        if not len(streams):
            raise ValueError("no streams")
        h, w, _ = jpeg_info(streams[0])
        keep, ptrs, sizes = self._jpeg_args(streams)
        out = np.empty((len(keep), h, w, 3), np.uint8)
        with self._lock:
            self._ck(self._L.ofk_jpeg_decode_bgr8(self._h, ptrs, sizes, len(keep), _p(out)))
        return out

    def jpeg_last_iterations(self):
        """Synchronisation passes the latest JPEG decode of this context queued behind the first (ofk_jpeg_last_iterations): 0 before any
        decode and for single-chunk streams."""
        with self._lock:
            return int(self._L.ofk_jpeg_last_iterations(self._h))

    def pairs_set_sensors(self, sensors):
        s = _arr(sensors, np.float64).reshape(-1, SENSOR_DOUBLES)
        with self._lock:
            self._ck(self._L.ofk_pairs_set_sensors(self._h, _p(s), len(s)))

    def pairs_run(self, params):
        with self._lock:
            self._ck(self._L.ofk_pairs_run(self._h, C.byref(params)))

    def pairs_download(self, points=True):
        B = self._resident[0]; S = self.max_pts
        rec = np.empty((B, RECORD_DOUBLES), np.float64)
        if points:
            pp = np.empty((B, S, 2), np.float32); npts = np.empty((B, S, 2), np.float32)
            st = np.empty((B, S), np.uint8); err = np.empty((B, S), np.float32)
        else:
            pp = npts = st = err = None
        cnt = np.empty(B, np.int32)
        with self._lock:
            self._ck(self._L.ofk_pairs_download(self._h, _p(rec), _p(pp), _p(npts), _p(st), _p(err), _p(cnt)))
        return dict(records=rec, prev_pts=pp, next_pts=npts, status=st, err=err, counts=cnt)

    def pairs_export_records_f32(self, device_ptr, batch):
        with self._lock:
            self._ck(self._L.ofk_pairs_export_records_f32(self._h, C.c_void_p(int(device_ptr)), int(batch)))

    # ------------------------------------------------------------------ video streams (persistent tracks on the device)
    def stream_begin(self, first_bgr, params):
        first_bgr, _ = self._batched(first_bgr, 3)
        first_bgr = _arr(first_bgr, np.uint8)
        B, h, w, ch = first_bgr.shape
        if ch != 3:
            raise ValueError("expected [B,h,w,3] BGR frames")
        mc = int(params.max_corners)
        tracks = np.zeros((B, mc, 2), np.float32); counts = np.zeros(B, np.int32)
        with self._lock:
            self._ck(self._L.ofk_stream_begin(self._h, _p(first_bgr), B, h, w, C.byref(params), _p(tracks), _p(counts)))
        self._stream = (B, h, w)
        return tracks, counts

    def stream_step(self, next_bgr, sensors, params, min_features, mask_radius):
        B, h, w = self._stream
        next_bgr, _ = self._batched(next_bgr, 3)
        next_bgr = _arr(next_bgr, np.uint8, (B, h, w, 3))
        sensors = _arr(sensors, np.float64).reshape(B, SENSOR_DOUBLES)
        mc = int(params.max_corners)
        rec = np.zeros((B, RECORD_DOUBLES), np.float64)
        tracks = np.zeros((B, mc, 2), np.float32); counts = np.zeros(B, np.int32)
        with self._lock:
            self._ck(self._L.ofk_stream_step(self._h, _p(next_bgr), _p(sensors), C.byref(params), int(min_features), int(mask_radius),
                                             _p(rec), _p(tracks), _p(counts)))
        return rec, tracks, counts

    def stream_begin_jpeg(self, streams, params):
        """stream_begin with one baseline JPEG stream per camera (CompressedImage payloads), decoded on the device."""
        h, w, _ = jpeg_info(streams[0])
        keep, ptrs, sizes = self._jpeg_args(streams)
        B, mc = len(keep), int(params.max_corners)
        tracks = np.zeros((B, mc, 2), np.float32); counts = np.zeros(B, np.int32)
        with self._lock:
            self._ck(self._L.ofk_stream_begin_jpeg(self._h, ptrs, sizes, B, C.byref(params), _p(tracks), _p(counts)))
        self._stream = (B, h, w)
        return tracks, counts

    def stream_step_jpeg(self, streams, sensors, params, min_features, mask_radius):
        B, h, w = self._stream
        if len(streams) != B:
            raise ValueError(f"expected {B} JPEG streams")
        keep, ptrs, sizes = self._jpeg_args(streams)
        sensors = _arr(sensors, np.float64).reshape(B, SENSOR_DOUBLES)
        mc = int(params.max_corners)
        rec = np.zeros((B, RECORD_DOUBLES), np.float64)
        tracks = np.zeros((B, mc, 2), np.float32); counts = np.zeros(B, np.int32)
        with self._lock:
            self._ck(self._L.ofk_stream_step_jpeg(self._h, ptrs, sizes, _p(sensors), C.byref(params), int(min_features), int(mask_radius),
                                                  _p(rec), _p(tracks), _p(counts)))
        return rec, tracks, counts

    # ------------------------------------------------------------------ resident per-stream filters + fused step
    def imu_reset(self, batch, state0=None):
        st = None if state0 is None else _arr(state0, np.float64, (IMU_STATE,))
        with self._lock:
            self._ck(self._L.ofk_imu_reset(self._h, _p(st), int(batch)))

    def imu_push(self, msgs, counts=None):
        """msgs [B, M, 15] (or [B, 15] for one message per stream); counts [B] (default: M each)."""
        m = _arr(msgs, np.float64)
        if m.ndim == 2:
            m = m[:, None, :]
        B, M, k = m.shape
        if k != IMU_MSG:
            raise ValueError(f"an IMU message has {IMU_MSG} fields")
        cn = np.full(B, M, np.int32) if counts is None else _arr(counts, np.int32, (B,))
        m = np.ascontiguousarray(m)
        with self._lock:
            self._ck(self._L.ofk_imu_push(self._h, _p(m), _p(cn), M, B))

    def imu_state(self, batch):
        st = np.empty((batch, IMU_STATE), np.float64); dv = np.empty((batch, 3), np.float64)
        with self._lock:
            self._ck(self._L.ofk_imu_state(self._h, _p(st), _p(dv), int(batch)))
        return st, dv

    def filter_configure(self, model, batch):
        """model: pipeline.FilterModel (F, B, H, Q, R, x0, P0)."""
        ns, nm, nc = model.ns, model.nm, model.nc
        F = _arr(model.F, np.float64, (ns, ns)); H = _arr(model.H, np.float64, (nm, ns)); Q = _arr(model.Q, np.float64, (ns, ns))
        R = _arr(model.R, np.float64, (nm, nm)); Bm = _arr(model.B, np.float64, (ns, nc)) if nc else None
        x0 = _arr(model.x0, np.float64, (ns,)); P0 = _arr(model.P0, np.float64, (ns, ns))
        with self._lock:
            self._ck(self._L.ofk_filter_configure(self._h, ns, nm, nc, _p(F), _p(Bm), _p(H), _p(Q), _p(R), _p(x0), _p(P0), int(batch)))
        self._kf_ns = ns

    def filter_state(self, batch):
        ns = self._kf_ns
        x = np.empty((batch, ns), np.float64); P = np.empty((batch, ns, ns), np.float64)
        with self._lock:
            self._ck(self._L.ofk_filter_state(self._h, _p(x), _p(P), int(batch)))
        return x, P

    def stream_step_fused(self, next_bgr, sensors, params, fusion, min_features, mask_radius):
        """ofk_stream_step_fused: returns (records [B,16], fused [B,8], tracks [B,mc,2], counts [B])."""
        B, h, w = self._stream
        sensors = _arr(sensors, np.float64).reshape(B, SENSOR_DOUBLES)
        mc = int(params.max_corners)
        rec = np.zeros((B, RECORD_DOUBLES), np.float64); fused = np.zeros((B, 8), np.float64)
        tracks = np.zeros((B, mc, 2), np.float32); counts = np.zeros(B, np.int32)
        if isinstance(next_bgr, (list, tuple)) and isinstance(next_bgr[0], (bytes, bytearray, memoryview)):
            if len(next_bgr) != B:
                raise ValueError(f"expected {B} JPEG streams")
            keep, ptrs, sizes = self._jpeg_args(next_bgr)
            with self._lock:
                self._ck(self._L.ofk_stream_step_fused_jpeg(self._h, ptrs, sizes, _p(sensors), C.byref(params), C.byref(fusion), int(min_features),
                                                            int(mask_radius), _p(rec), _p(fused), _p(tracks), _p(counts)))
        else:
            frames, _ = self._batched(next_bgr, 3)
            frames = _arr(frames, np.uint8, (B, h, w, 3))
            with self._lock:
                self._ck(self._L.ofk_stream_step_fused(self._h, _p(frames), _p(sensors), C.byref(params), C.byref(fusion), int(min_features),
                                                       int(mask_radius), _p(rec), _p(fused), _p(tracks), _p(counts)))
        return rec, fused, tracks, counts

    def pairs_filter_step(self, batch, z_sign=-1.0, z_source=0):
        """Per-pair resident filter update behind the latest pairs_run (asynchronous)."""
        with self._lock:
            self._ck(self._L.ofk_pairs_filter_step(self._h, float(z_sign), int(z_source), int(batch)))

    def stream_last_points(self, stride):
        """(next_pts [B,stride,2] f32, keep [B,stride] u8) of the latest stream step."""
        B = self._stream[0]
        nxt = np.zeros((B, stride, 2), np.float32); keep = np.zeros((B, stride), np.uint8)
        with self._lock:
            self._ck(self._L.ofk_stream_last_points(self._h, _p(nxt), _p(keep), int(stride)))
        return nxt, keep

    # ------------------------------------------------------------------ multi-GPU exchange (RCCL through the library, no torch)
    def comm_init(self, unique_id, rank, world):
        uid = np.frombuffer(bytes(unique_id), np.uint8).copy()
        if uid.size == 0 or uid.size % 128:
            raise ValueError("RCCL unique ids have 128 bytes each")
        with self._lock:
            self._ck(self._L.ofk_comm_init(self._h, _p(uid), uid.size // 128, int(rank), int(world)))
        self.comm_rank, self.comm_world = int(rank), int(world)

    def comm_add(self, unique_id):
        """One more communicator (128-byte id).  Collective: every rank calls it, in the same order; an error is fatal for the job."""
        uid = np.frombuffer(bytes(unique_id), np.uint8).copy()
        if uid.size != 128:
            raise ValueError("one 128-byte RCCL unique id")
        with self._lock:
            self._ck(self._L.ofk_comm_add(self._h, _p(uid)))

    def comm_destroy(self):
        with self._lock:
            self._ck(self._L.ofk_comm_destroy(self._h))

    def comm_gather_records(self, batch, slot=0):
        """Queues the all-gather of the latest step's [batch, 8] f32 records behind that step; returns at once."""
        with self._lock:
            self._ck(self._L.ofk_comm_gather_records(self._h, int(batch), int(slot)))

    def comm_fetch_records(self, batch, slot=0):
        out = np.empty((self.comm_world, int(batch), 8), np.float32)
        with self._lock:
            self._ck(self._L.ofk_comm_fetch_records(self._h, int(slot), int(batch), _p(out)))
        return out

    def comm_count(self):
        """Communicators the ranks agreed on (1 = one gather per step behind the last slice)."""
        return int(self._L.ofk_comm_count(self._h))

    def comm_pending(self, slot=0):
        """Non-blocking: bitmask of the slices whose gather of `slot` has not completed (watchdogs)."""
        return int(self._L.ofk_comm_pending(self._h, int(slot)))

    def comm_allreduce(self, values, op="sum"):
        v = np.ascontiguousarray(np.atleast_1d(values), np.float64).copy()
        with self._lock:
            self._ck(self._L.ofk_comm_allreduce_f64(self._h, _p(v), v.size, {"sum": 0, "max": 1, "min": 2}[op]))
        return v

    def set_overlap(self, on):
        self._ck(self._L.ofk_set_overlap(self._h, 1 if on else 0))

    def mark(self, slot=0):
        """Records a completion mark behind everything queued on the context's stream (slots 0..7)."""
        self._ck(self._L.ofk_mark(self._h, int(slot)))

    def mark_wait(self, slot=0):
        """Blocks the host until mark `slot` has been reached; later work keeps running."""
        self._ck(self._L.ofk_mark_wait(self._h, int(slot)))

    def set_streams(self, n):
        self._ck(self._L.ofk_set_streams(self._h, int(n)))

    def profile_enable(self, mask):
        self._ck(self._L.ofk_profile_enable(self._h, int(mask)))

    def resident_pyramid(self, frame_set, image, h, w, levels):
        """The resident pyramid of one image (frame set 0 = previous, 1 = next frames of the latest pairs batch, or the stream
        loop's slot): list of uint8 arrays, level 0 = the gray frame."""
        shapes, offs, off = [], [], 0
        for l in range(levels + 1):
            shapes.append((h, w)); offs.append(off)
            off += (h * w + 255) // 256 * 256
            h, w = (h + 1) // 2, (w + 1) // 2
        buf = np.empty(off, np.uint8)
        with self._lock:
            self._ck(self._L.ofk_resident_pyramid(self._h, int(frame_set), int(image), _p(buf), buf.size))
        return [buf[o:o + a * b].reshape(a, b).copy() for (a, b), o in zip(shapes, offs)]

    def profile_read(self):
        ms = np.zeros(len(STAGES), np.float64); n = np.zeros(len(STAGES), np.int32)
        with self._lock:
            self._ck(self._L.ofk_profile_read(self._h, _p(ms), _p(n)))
        return {s: (float(ms[i]), int(n[i])) for i, s in enumerate(STAGES)}


def comm_unique_id(n_ids=1):
    """n_ids x 128-byte RCCL unique ids (call on rank 0, hand to every rank): one communicator per free-running slice."""
    uid = np.zeros(128 * int(n_ids), np.uint8)
    rc = load_library().ofk_comm_unique_id(_p(uid), int(n_ids))
    if rc != OK:
        raise OfkError(rc, load_library().ofk_last_error(None).decode())
    return uid.tobytes()


def comm_reorder_records(recv, world, batch, slices):
    """Host-only: the per-slice receive order of ofk_comm_gather_records -> rank-major [world, batch, 8] (ofk_comm_fetch_records'
    reassembly, callable without a GPU)."""
    recv = np.ascontiguousarray(recv, np.float32)
    out = np.empty((int(world), int(batch), 8), np.float32)
    L = load_library()
    if recv.size != out.size or L.ofk_comm_reorder_records(_p(recv), int(world), int(batch), int(slices), _p(out)) != OK:
        raise OfkError(E_INVALID, "comm_reorder_records: bad argument")
    return out


def set_tuning(knob, value):
    """Launch-geometry knob for measurements (ofk_set_tuning in include/ofk.h); 0 restores the built-in choice.  Process-wide."""
    L = load_library()
    if L.ofk_set_tuning(str(knob).encode(), int(value)) != OK:
        raise OfkError(E_INVALID, L.ofk_last_error(None).decode())


def get_tuning(knob):
    L = load_library()
    v = C.c_int(0)
    if L.ofk_get_tuning(str(knob).encode(), C.byref(v)) != OK:
        raise OfkError(E_INVALID, L.ofk_last_error(None).decode())
    return v.value


def _seed_mode(mode):
    if isinstance(mode, str):
        if mode not in SEED_MODES:
            raise ValueError(f"seed mode {mode!r} is none of {sorted(SEED_MODES)}")
        return SEED_MODES[mode]
    return int(mode)


def make_sensors(batch, d=1.0, normal=(0, 0, 1), omega=(0, 0, 0), rotation=None, offset=(0, 0, 0.1), scaling=0.01,
                 cx=0.0, cy=0.0, v_prior=(0, 0, 0)):
    """Builds the [batch][28] sensor records ofk_pairs_set_sensors takes (layout: include/ofk.h)."""
    s = np.zeros((batch, SENSOR_DOUBLES), np.float64)
    s[:, 0] = d; s[:, 1:4] = normal; s[:, 4:7] = omega
    s[:, 7:16] = np.eye(3).ravel() if rotation is None else np.asarray(rotation, np.float64).reshape(-1, 9)
    s[:, 16:19] = offset; s[:, 19] = scaling; s[:, 20] = cx; s[:, 21] = cy; s[:, 22:25] = v_prior
    return s


_default = None
_default_lock = threading.Lock()


def default_context(min_w=0, min_h=0, min_pts=0, min_level=0):
    """Process-wide context used by the of_library / cv2-style facade; grown on demand."""
    global _default
    with _default_lock:
        c = _default
        if c is None or c.max_w * c.max_h < min_w * min_h or c.max_pts < min_pts or c.max_level < min_level:
            w = max(min_w, c.max_w if c else 1920); h = max(min_h, c.max_h if c else 1080)
            pts = max(min_pts, c.max_pts if c else 512); lvl = max(min_level, c.max_level if c else 5)
            # build the bigger context FIRST: if that fails (a corrupt JPEG header asking for 65535 x 65535, out of memory) the
            # old one stays in place and the facade keeps working
            new = Context(int(os.environ.get("OFK_DEVICE", "0")), w, h, 1, pts, lvl)
            _default = new
            if c is not None:
                c.close()
        return _default
