"""velocity_node.py — the reference's ROS node `velocity_measurment_node`, with its numpy loops and (commented-out)
OpenCV calls running on the HIP kernels.

Module level: generate_test_data (node:25-29), solve_lgs (node:30-42), feasible (node:44-50).
Class optical_fusion (node:52-267): same attributes, flags, callbacks (call_dist / call_imu / call_optical), topic
names and printed output.  Differences, all deliberate:
  * rospy is optional: `optical_fusion(spin=False)` builds the state without ROS so the node logic is testable;
    `step()` is one iteration of the reference's busy loop (node:226-267).
  * `synthetic_test=True` (default) reproduces the node AS SHIPPED: 4 hard-coded features (node:123), flow
    overwritten by generate_test_data (node:236), feasibility forced to -1 (node:240).  With
    `synthetic_test=False` the pipeline the reference keeps inside ''' blocks runs instead — on the DEVICE-RESIDENT
    stream loop (pipeline.FlowStream, ofk_stream_step_fused): the CompressedImage payload is decoded on the GPU, gray
    levels / pyramids / tracks never leave HBM, and one callback = JPEG decode, goodFeaturesToTrack on the first frame
    (node:120) or calcOpticalFlowPyrLK from the resident tracks (node:133-136), the real flow, the real r_tilde filter,
    solve_lgs, lever arm (node:229-258) and the re-detection with a circle mask (node:157-173); step() publishes it.
  * callbacks and step() snapshot shared state under one lock (the reference races, node:61-177 vs :226-267).
"""
import copy
import os
import threading
import time

import numpy as np

try:
    from . import ofk, cv2_hip as cv2, of_library as of
    from .pipeline import CameraModel, FlowStream, FusionConfig, PipelineConfig, RollingShutter
except ImportError:
    import ofk
    import cv2_hip as cv2
    import of_library as of
    from pipeline import CameraModel, FlowStream, FusionConfig, PipelineConfig, RollingShutter

try:                                    # ROS is optional (absent in this image)
    import rospy
    from cv_bridge import CvBridge
    from sensor_msgs.msg import CompressedImage, Image, Imu, Range
except ImportError:
    rospy = None
    CvBridge = CompressedImage = Image = Imu = Range = None


def generate_test_data(x, v, omega, d, n):
    """node:25-29 — forward flow model, one thread per point (k_flow_model)."""
    x = np.asarray(x, np.float64)
    if len(x) == 0:
        return np.zeros((0, 2))
    return ofk.default_context().flow_model(x[:, :2], v, omega, float(d), n)


def solve_lgs(x, u, d, n, omega):
    """node:30-42 — returns np.linalg.lstsq's 4-tuple (v, R, rank, s): R has shape (1,) when rank == 3 and
    3N > 3, else is empty.  On failure the reference returns the 2-tuple (zeros(3), 10000*ones(3N)) from a bare
    except (node:41-42); that path is kept for non-finite results."""
    x = np.asarray(x, np.float64); u = np.asarray(u, np.float64)
    out = ofk.default_context().velocity_solve(ofk.SOLVE_NODE, x[:, :2], u[:, :2], d=float(d), nrm=n, omega=omega)
    if not np.all(np.isfinite(out)):
        return np.zeros(3), 10000 * np.ones(3 * len(x))
    rank = int(out[4])
    R = np.array([out[3]]) if (rank == 3 and 3 * len(x) > 3) else np.empty(0)
    return out[:3].copy(), R, rank, out[5:8].copy()


def solve_lgs_robust(x, u, d, n, omega, **settings):
    """solve_lgs with the robust estimator of ofk.h (ofk_velocity_solve_robust): a sampled least-median-of-squares start, then
    reweighting rounds.  settings: ofk.robust_setting's keywords (loss="tukey", c, iters, hypotheses, seed).
    Returns (v, R, rank, s, weights [N], stats [8]): R = the weighted residual sum (shape (1,) when rank == 3 and 3N > 3)."""
    x = np.asarray(x, np.float64); u = np.asarray(u, np.float64)
    out, w, st = ofk.default_context().velocity_solve_robust(ofk.SOLVE_NODE, x[:, :2], u[:, :2], d=float(d), nrm=n, omega=omega, **settings)
    rank = int(out[4])
    R = np.array([out[3]]) if (rank == 3 and 3 * len(x) > 3) else np.empty(0)
    return out[:3].copy(), R, rank, out[5:8].copy(), w, st


def solve_lgs_cov(x, u, d, n, omega, mode="propagate", **sigmas):
    """solve_lgs with the covariance of its result (ofk.h: ofk_velocity_solve_cov): first-order propagation of the input sigmas
    through the solve.  sigmas: ofk.cov_setting's keywords (sigma_flow, sigma_pos in the units of x and u; sigma_d; sigma_omega;
    sigma_normal); mode "residual" takes the flow and position terms from the solve's own residual.
    Returns (v, R, rank, s, C_v [3,3], cov [24]); C_v is zero and cov[13] == 1 where there is no covariance (rank < 3)."""
    x = np.asarray(x, np.float64); u = np.asarray(u, np.float64)
    out, cov = ofk.default_context().velocity_solve_cov(ofk.SOLVE_NODE, x[:, :2], u[:, :2], d=float(d), nrm=n, omega=omega, mode=mode, **sigmas)
    rank = int(out[4])
    R = np.array([out[3]]) if (rank == 3 and 3 * len(x) > 3) else np.empty(0)
    return out[:3].copy(), R, rank, out[5:8].copy(), ofk.cov_matrix(cov[0:6]), cov


def gyro_bias_step(x, u, d, n, omega_raw, state=None, **settings):
    """One step of a stream's gyro bias without images (ofk.h: ofk_gyro_bias_step): solve_lgs at omega_raw less the bias, then the
    filter step that refines the bias from the flow.  state: the [32] returned by the previous call (None: the setting's start);
    settings: ofk.gyro_bias_setting's keywords, sigma_flow in the units of x and u.
    Returns (v, R, rank, s, state [32]); state[0:3] is the bias, state[12:15] the omega the solve used, state[18] the flag."""
    x = np.asarray(x, np.float64); u = np.asarray(u, np.float64)
    out, st = ofk.default_context().gyro_bias_step(ofk.SOLVE_NODE, x[:, :2], u[:, :2], d=float(d), nrm=n, omega=omega_raw, state=state, **settings)
    rank = int(out[4])
    R = np.array([out[3]]) if (rank == 3 and 3 * len(x) > 3) else np.empty(0)
    return out[:3].copy(), R, rank, out[5:8].copy(), st


def _struct_field(name, value, **beside):
    """One per-track setting of optical_fusion.__init__ as the PipelineConfig field it becomes: None / False -> {} (off); True, the
    ofk structure or a dict of ofk.<name>_setting's keywords -> {name: True or the structure}.  Invalid fields fail here, not at the
    first frame: the field goes through PipelineConfig(**beside, name=...).<name>_setting() once."""
    if value is None or value is False:
        return {}
    field = {name: value if value is True or isinstance(value, dict(ofk.SETTINGS)[name]) else getattr(ofk, name + "_setting")(**dict(value))}
    getattr(PipelineConfig(**beside, **field), name + "_setting")()
    return field


# optical_fusion.last_<name>: the FlowStream reader and the keys it publishes
_LAST_PER_TRACK = {
    "track_depth": (FlowStream.depths, ("rho", "var", "nobs", "ids", "rec")),
    "keyframe": (FlowStream.position, ("pos", "D", "T", "flag", "C_T", "R_acc", "live", "members_at_key", "key_step", "keyframes", "dead_reckoned",
                                       "reason", "ids", "rec")),
    "keyframe_rotation": (FlowStream.key_rotation, ("delta", "R_hat", "C_delta", "flag", "prior", "eig", "iterations", "rec")),
    "track_template": (FlowStream.templates, ("A", "ncc", "flag", "tstate", "ids", "rec")),
}


def track_depth_step(x, u, omega, v, state=None, status=None, solved=True, new_count=None, max_total=None, **settings):
    """One step of a stream's depths per track without images (ofk.h: ofk_track_depth_step): the map solve from the depths in
    `state`, then measurement, prediction and compaction.  x, u [n,2]: the solve's points and flow; omega, v: what the step's solve
    read and returned; state: the dict(rho, var, nobs) of the previous call (None: no depth yet); status [n] (None: all kept);
    new_count: corners re-detected behind the kept rows; max_total: the most rows the stream holds (None: whatever fits); settings:
    ofk.track_depth_setting's keywords, sigma_flow and b_min in the units of x and u.
    Returns (state, rec [32]): the kept rows in order and the appended ones behind them; rec[0:3] is v_map, rec[3] its flag."""
    x = np.asarray(x, np.float64).reshape(-1, 2); u = np.asarray(u, np.float64).reshape(-1, 2)
    n = len(x)
    if n < 1:
        raise ValueError("track_depth_step: no points")
    st = np.ones(n, np.uint8) if status is None else (np.asarray(status).reshape(n) != 0).astype(np.uint8)
    kept, born = int(st.sum()), 0 if new_count is None else max(int(new_count), 0)
    S = max(n, kept + born)                                      # room for the appended rows
    if max_total is not None:
        born = max(0, min(born, int(max_total) - kept))

    def rows(a, dtype, *tail):                                   # [1, S, ...]: the n rows, zeros behind them
        out = np.zeros((1, S) + tail, dtype)
        if a is not None:
            out[0, :n] = np.asarray(a, dtype).reshape((n,) + tail)
        return out
    state = state or {}
    out, rec = ofk.default_context().track_depth_step(
        rows(x, np.float64, 2), rows(u, np.float64, 2), rows(st, np.uint8), [n], [omega], [v], [1 if solved else 0],
        dict(rho=rows(state.get("rho"), np.float64), var=rows(state.get("var"), np.float64), nobs=rows(state.get("nobs"), np.int32)),
        new_counts=None if new_count is None else [born], max_total=S, **settings)
    return {k: a[0, :kept + born].copy() for k, a in out.items()}, rec[0]


def _keyframe_stage(who, next_pts, sensors, v_uav, state, status, solved, step, new_count, max_total):
    """What keyframe_step and keyframe_rotation_step hand to their stage entry: the one stream's rows padded to a batch of one with room
    for the appended rows.  -> (the positional arguments up to the state dict, keywords new_counts / max_total, rows kept + born)."""
    pts = np.asarray(next_pts, np.float32).reshape(-1, 2)
    n = len(pts)
    if n < 1:
        raise ValueError(f"{who}: no points")
    st = np.ones(n, np.uint8) if status is None else (np.asarray(status).reshape(n) != 0).astype(np.uint8)
    kept, born = int(st.sum()), 0 if new_count is None else max(int(new_count), 0)
    S = max(n, kept + born)                                      # room for the appended rows
    if max_total is not None:
        born = max(0, min(born, int(max_total) - kept))

    def rows(a, dtype, *tail):                                   # [1, S, ...]: the n rows, zeros behind them
        out = np.zeros((1, S) + tail, dtype)
        if a is not None:
            out[0, :n] = np.asarray(a, dtype).reshape((n,) + tail)
        return out
    state = state or {}
    sd = np.zeros((1, ofk.KEY_STATE)); sd[0, [0, 4, 8]] = 1.0
    if state.get("state") is not None:
        sd[0] = np.asarray(state["state"], np.float64).reshape(ofk.KEY_STATE)
    si = np.zeros((1, ofk.KEY_INTS), np.int32) if state.get("istate") is None else np.asarray(state["istate"], np.int32).reshape(1, ofk.KEY_INTS)
    rs = None if state.get("rstate") is None else np.asarray(state["rstate"], np.float64).reshape(1, ofk.KEYROT_STATE)
    args = (rows(pts, np.float32, 2), rows(st, np.uint8), [n], np.asarray(sensors, np.float64).reshape(1, ofk.SENSOR_DOUBLES), [v_uav],
            [1 if solved else 0], [int(step)], dict(key_xy=rows(state.get("key_xy"), np.float32, 2), member=rows(state.get("member"), np.uint8),
                                                      state=sd, istate=si, rstate=rs))
    return args, dict(new_counts=None if new_count is None else [born], max_total=S), kept + born


def _keyframe_state(out, count):
    """The one stream's state of a stage entry's batch of one: the kept rows in order and the appended ones behind them."""
    res = dict(key_xy=out["key_xy"][0, :count].copy(), member=out["member"][0, :count].copy(), state=out["state"][0].copy(),
               istate=out["istate"][0].copy())
    if "rstate" in out:
        res["rstate"] = out["rstate"][0].copy()
    return res


def keyframe_step(next_pts, sensors, v_uav=(0.0, 0.0, 0.0), state=None, status=None, solved=True, step=0, new_count=None, max_total=None,
                  **settings):
    """One step of a stream's keyframe without images (ofk.h: ofk_keyframe_step): rotate, key solve, position, re-key decision and
    compaction.  next_pts [n,2]: the ideal next points in pixels; sensors [28]: the step's sensor row; v_uav, solved: the step
    record's fields 8-10 and its solved flag (the dead reckoning without a key solve); state: the dict(key_xy, member, state, istate)
    of the previous call (None: no keyframe yet, position zero); status [n] (None: all kept); step: the track table's step;
    new_count: corners re-detected behind the kept rows; max_total: the most rows the stream holds (None: whatever fits); settings:
    ofk.keyframe_setting's keywords.
    Returns (state, rec [32]): the kept rows in order and the appended ones behind them; rec[13:16] is the position, rec[3] the flag."""
    args, kw, count = _keyframe_stage("keyframe_step", next_pts, sensors, v_uav, state, status, solved, step, new_count, max_total)
    out, rec = ofk.default_context().keyframe_step(*args, **kw, **settings)
    return _keyframe_state(out, count), rec[0]


def keyframe_rotation_step(next_pts, sensors, v_uav=(0.0, 0.0, 0.0), state=None, status=None, solved=True, step=0, new_count=None,
                           max_total=None, keyframe=None, rotation=None):
    """keyframe_step with the accumulated rotation refined from the flow (ofk.h: ofk_keyframe_rotation_step).  keyframe_step's
    arguments; state may also carry rstate [12]; keyframe / rotation: None (the defaults), a dict of ofk.keyframe_setting's /
    ofk.keyframe_rotation_setting's keywords, or the structures.
    Returns (state with rstate, rec [32], rrec [40]): rrec[0:3] is the correction, rrec[3] its flag (ofk.KEYROT_*)."""
    kf = keyframe if isinstance(keyframe, ofk.Keyframe) else ofk.keyframe_setting(**dict(keyframe or {}))
    rot = rotation if isinstance(rotation, ofk.KeyframeRotation) else ofk.keyframe_rotation_setting(**dict(rotation or {}))
    args, kw, count = _keyframe_stage("keyframe_rotation_step", next_pts, sensors, v_uav, state, status, solved, step, new_count, max_total)
    out, rec, rrec = ofk.default_context().keyframe_rotation_step(*args, **kw, keyframe=kf, rotation=rot)
    return _keyframe_state(out, count), rec[0], rrec[0]


def keyframe_map_step(next_pts, sensors, v_uav=(0.0, 0.0, 0.0), state=None, depth=None, status=None, solved=True, step=0, new_count=None,
                      max_total=None, keyframe=None, keyframe_map=None):
    """keyframe_step with the key translation solved against the per-track depths frozen at the keyframe (ofk.h:
    ofk_keyframe_map_step).  keyframe_step's arguments; state may also carry key_rho, key_var [n] and mstate [2]; depth: the
    dict(rho, var, nobs) [n] track_depth_step returned for the previous step (None: no depth state); keyframe / keyframe_map: None
    (the defaults), a dict of ofk.keyframe_setting's / ofk.keyframe_map_setting's keywords, or the structures.
    Returns (state with key_rho, key_var, mstate; rec [32]; mrec [32]): mrec[0] is the map's flag (ofk.KEYMAP_*)."""
    kf = keyframe if isinstance(keyframe, ofk.Keyframe) else ofk.keyframe_setting(**dict(keyframe or {}))
    km = keyframe_map if isinstance(keyframe_map, ofk.KeyframeMap) else ofk.keyframe_map_setting(**dict(keyframe_map or {}))
    args, kw, count = _keyframe_stage("keyframe_map_step", next_pts, sensors, v_uav, state, status, solved, step, new_count, max_total)
    n, S = int(args[2][0]), args[0].shape[1]

    def rows(a, dtype):                                          # [1, S]: the n rows, zeros behind them
        out = np.zeros((1, S), dtype)
        if a is not None:
            out[0, :n] = np.asarray(a, dtype).reshape(n)
        return out
    state = state or {}
    st = dict(args[-1], key_rho=rows(state.get("key_rho"), np.float64), key_var=rows(state.get("key_var"), np.float64),
              mstate=None if state.get("mstate") is None else np.asarray(state["mstate"], np.int32).reshape(1, 2))
    st.pop("rstate", None)
    dp = None if depth is None else dict(rho=rows(depth["rho"], np.float64), var=rows(depth["var"], np.float64), nobs=rows(depth["nobs"], np.int32))
    out, rec, mrec = ofk.default_context().keyframe_map_step(*args[:-1], st, depth=dp, **kw, keyframe=kf, keyframe_map=km)
    res = _keyframe_state(out, count)
    res.update(key_rho=out["key_rho"][0, :count].copy(), key_var=out["key_var"][0, :count].copy(), mstate=out["mstate"][0].copy())
    return res, rec[0], mrec[0]


def stabilise_step(R, key_rec, sensors, h, w, state=None, normal=None, prev_covered=None, **settings):
    """One step of a stream's stabilised view without images (ofk.h: ofk_stab_pose): the pixel homography M that warps the step's
    frame into the view, and the view kept across re-keys.  R [3,3]: the rotation the key solve used; key_rec [32]: the keyframe's
    record of the step; sensors [28]: the step's sensor row; h, w: the frame; state: the dict the previous call returned (None: the
    identity); normal [3]: the IMU state's normal under use_imu (None: the sensor row's); prev_covered: the covered pixels of the
    previous warp (None: none yet); settings: ofk.stabilise_setting's keywords.
    Returns (state dict(Bv [3,3], ints [4]), rec [48]): rec[0:9] is M, rec[30] the flag (ofk.STAB_*), rec[31] the re-base reason."""
    st = None
    if state is not None:
        st = dict(Bv=np.asarray(state["Bv"], np.float64).reshape(1, 3, 3), ints=np.array(state["ints"], np.int32).reshape(1, ofk.STAB_INTS))
        st["ints"][0, 3] = 0 if prev_covered is None else 1
    out, rec = ofk.default_context().stab_pose(np.asarray(R, np.float64).reshape(1, 3, 3), np.asarray(key_rec, np.float64).reshape(1, ofk.KEY_DOUBLES),
                                               np.asarray(sensors, np.float64).reshape(1, ofk.SENSOR_DOUBLES), h, w, state=st,
                                               normal=None if normal is None else np.asarray(normal, np.float64).reshape(1, 3),
                                               prev_covered=None if prev_covered is None else [int(prev_covered)], **settings)
    return dict(Bv=out["Bv"][0], ints=out["ints"][0]), rec[0]


def rectify_frame(frame, camera, M=None, dsize=None, border="constant", border_value=0, r_max=0.0):
    """A raw frame of `camera` (a pipeline.CameraModel, an ofk.Camera or a dict of CameraModel's fields) rectified on the device (ofk.h:
    ofk_warp_lens): frame [h,w] or [h,w,3] uint8; M [3,3] maps a pixel of the output to an IDEAL pixel of the camera (None: the identity,
    cv2.undistort's result); dsize (height, width), None = the frame's; r_max: ideal normalised radius beyond which a pixel is border,
    e.g. 1.05 * camera.ideal_radius(h, w).  Returns (image in the frame's layout, covered pixels)."""
    cam = camera if isinstance(camera, ofk.Camera) else (camera if isinstance(camera, CameraModel) else CameraModel(**dict(camera))).setting()
    frame = np.asarray(frame, np.uint8)
    h, w = frame.shape[:2] if dsize is None else dsize
    return ofk.default_context(max(int(w), frame.shape[1]), max(int(h), frame.shape[0])).warp_lens(frame, cam, M, dsize, border, border_value, r_max)


def pos_filter_step(v_uav, key_rec, R_world=None, state=None, solved=True, du=None, fix=None, fix_sigma=None, **settings):
    """One step of a stream's position filter without images (ofk.h: ofk_pos_filter_step): predict, the velocity, displacement and fix
    updates, the clone at a re-key.  v_uav [3], solved: the step record's fields 8-10 and its solved flag; key_rec [32]: the
    keyframe's record of the step (keyframe_step's rec); R_world [3,3] (None: the identity); state: the dict(x, P, istate) of the
    previous call (None: not started, at zero; dict(x=[px, py, pz, 0, ...]) starts elsewhere); du [3]: the velocity increment of
    the step; fix [3] with fix_sigma (a number or [3]): an absolute position; settings: ofk.pos_filter_setting's keywords.
    Returns (state, rec [48]): rec[0:3] is the position, rec[25], rec[30], rec[35] the updates' outcomes (ofk.POSF_*)."""
    inp = np.zeros((1, ofk.POSF_INPUT), np.float64)
    if du is not None:
        inp[0, 0:3] = np.asarray(du, np.float64).reshape(3)
    if fix is not None:
        if fix_sigma is None:
            raise ValueError("pos_filter_step: a fix needs fix_sigma")
        inp[0, 3] = 1.0
        inp[0, 4:7] = np.asarray(fix, np.float64).reshape(3)
        inp[0, 7:10] = np.broadcast_to(np.asarray(fix_sigma, np.float64), (3,))
    st = None if state is None else {k: None if state.get(k) is None else np.asarray(state[k])[None] for k in ("x", "P", "istate")}
    rw = np.eye(3) if R_world is None else np.asarray(R_world, np.float64).reshape(3, 3)
    out, rec = ofk.default_context().pos_filter_step(np.asarray(v_uav, np.float64).reshape(1, 3), [1 if solved else 0],
                                                     np.asarray(key_rec, np.float64).reshape(1, ofk.KEY_DOUBLES), rw[None], state=st, input=inp,
                                                     **settings)
    return {k: a[0].copy() for k, a in out.items()}, rec[0]


def track_template_step(prev, next, prev_pts, next_pts, state=None, status=None, age=None, L=None, new_count=None, max_total=None, **settings):
    """One step of a stream's track templates on two gray frames (ofk.h: ofk_track_affine_fit, ofk_track_template_step): the step map
    fitted to the tracked rows (unless L [4] is given), then capture, score, re-anchoring, verdict and compaction.  prev, next [h,w]
    u8; prev_pts, next_pts [n,2]: LK's; state: the dict(tmpl, A, ncc, flag, tstate) of the previous call (None: no template yet);
    status [n] (None: all tracked); age [n] (None: 1 where the state has rows, else 0); new_count: corners re-detected behind the
    kept rows; settings: ofk.track_template_setting's keywords.
    Returns (next_pts [n,2], status [n], state, rec [32]): the rows as tracked with the corrected positions and the verdicts' status,
    the state of the kept rows in order with the appended ones behind them."""
    pp = np.asarray(prev_pts, np.float32).reshape(-1, 2); nn = np.asarray(next_pts, np.float32).reshape(-1, 2)
    n = len(pp)
    if n < 1:
        raise ValueError("track_template_step: no points")
    tp = ofk.track_template_setting(**settings)
    ts = ofk.tpl_stride(tp.win)
    st = np.ones(n, np.uint8) if status is None else (np.asarray(status).reshape(n) != 0).astype(np.uint8)
    born = 0 if new_count is None else max(int(new_count), 0)
    S = n + born                                                 # room for the appended rows
    state = state or {}
    have = len(state["tstate"]) if "tstate" in state else 0

    def rows(a, dtype, *tail):                                   # [1, S, ...]: the n rows, zeros behind them
        out = np.zeros((1, S) + tail, dtype)
        if a is not None:
            a = np.asarray(a, dtype).reshape((-1,) + tail)[:n]
            out[0, :len(a)] = a
        return out
    ag = rows((np.arange(n) < have).astype(np.int32) if age is None else age, np.int32)
    ctx = ofk.default_context()
    g0 = np.ascontiguousarray(prev, np.uint8)[None]; g1 = np.ascontiguousarray(next, np.uint8)[None]
    rec1 = np.zeros(ofk.TPL_DOUBLES)
    if L is None:
        r, Lf = ctx.track_affine_fit(rows(pp, np.float32, 2), rows(nn, np.float32, 2), rows(st, np.uint8), [n], g0.shape[1], g0.shape[2], tp)
        rec1, L = r[0], Lf[0]
    nx, so, out, rec = ctx.track_template_step(
        g0, g1, rows(pp, np.float32, 2), rows(nn, np.float32, 2), rows(st, np.uint8), ag, [n], np.asarray(L, np.float32).reshape(1, 4),
        dict(tmpl=rows(state.get("tmpl"), np.uint8, ts), A=rows(state.get("A"), np.float32, 4), ncc=rows(state.get("ncc"), np.float32),
             flag=rows(state.get("flag"), np.uint8), tstate=rows(state.get("tstate"), np.uint8)),
        new_counts=None if new_count is None else [born], max_total=S if max_total is None else min(int(max_total), S), track_template=tp)
    kept = int((so[0, :n] != 0).sum())
    total = kept + (0 if new_count is None else max(0, min(born, (S if max_total is None else min(int(max_total), S)) - kept)))
    rec = rec[0].copy(); rec[:10] = rec1[:10]
    return nx[0, :n].copy(), so[0, :n].copy(), {k: a[0, :total].copy() for k, a in out.items()}, rec


def solve_lgs_joint(x, u, d, n, omega, sigma_flow, sigma_omega=None):
    """solve_lgs with the gyro refined from the flow (ofk.h: ofk_velocity_solve_joint): velocity and rotation from one 6-unknown
    least squares.  sigma_flow: the flow noise in the units of x and u; sigma_omega: None (every axis free), a scalar or three
    values - the prior on omega's error (inf: free, 0: held).
    Returns (v, R, rank, s, omega_hat, joint [32]); joint[10] != 0 where the joint solve left the plain result alone."""
    x = np.asarray(x, np.float64); u = np.asarray(u, np.float64)
    out, jr = ofk.default_context().velocity_solve_joint(ofk.SOLVE_NODE, x[:, :2], u[:, :2], d=float(d), nrm=n, omega=omega,
                                                         sigma_flow=sigma_flow, sigma_omega=sigma_omega)
    rank = int(out[4])
    R = np.array([out[3]]) if (rank == 3 and 3 * len(x) > 3) else np.empty(0)
    return out[:3].copy(), R, rank, out[5:8].copy(), jr[0:3].copy(), jr


def solve_lgs_plane(x, u, d, n, omega, sigma_flow, sigma_normal=None, **settings):
    """solve_lgs with the ground normal refined from the flow (ofk.h: ofk_velocity_solve_plane): velocity and the plane's tilt from
    one 5-unknown Gauss-Newton iteration, the range along the beam held.  sigma_flow: the flow noise in the units of x and u;
    sigma_normal: None (the tilt is free) or the prior's standard deviation in radians (0: held); settings: sigma_max, beam, iters of
    ofk.plane_setting.
    Returns (v, R, rank, s, n_hat, d_hat, plane [32]); plane[10] != 0 where the plane solve left the plain result alone."""
    x = np.asarray(x, np.float64); u = np.asarray(u, np.float64)
    out, pr = ofk.default_context().velocity_solve_plane(ofk.SOLVE_NODE, x[:, :2], u[:, :2], d=float(d), nrm=n, omega=omega,
                                                         sigma_flow=sigma_flow, sigma_normal=sigma_normal, **settings)
    rank = int(out[4])
    R = np.array([out[3]]) if (rank == 3 and 3 * len(x) > 3) else np.empty(0)
    return out[:3].copy(), R, rank, out[5:8].copy(), pr[0:3].copy(), float(pr[3]), pr


def solve_lgs_epipolar(x, u, d, n, omega, **settings):
    """solve_lgs over ground that is no plane (ofk.h: ofk_velocity_solve_epipolar): the direction of v from the epipolar constraint,
    its length from the range at the beam's foot, one inverse depth per point.  settings: anchor (in the units of x), anchor_min,
    sigma_max, beam, weights of ofk.epipolar_setting.
    Returns (v, R, rank, s, rho [N], epi [32], points [N,4]); epi[10] != 0 where the epipolar solve left the plain result alone."""
    x = np.asarray(x, np.float64); u = np.asarray(u, np.float64)
    out, er, pts = ofk.default_context().velocity_solve_epipolar(ofk.SOLVE_NODE, x[:, :2], u[:, :2], d=float(d), nrm=n, omega=omega, **settings)
    rank = int(out[4])
    R = np.array([out[3]]) if (rank == 3 and 3 * len(x) > 3) else np.empty(0)
    return out[:3].copy(), R, rank, out[5:8].copy(), pts[:, 0].copy(), er, pts


def finite_points(prev, next, sensors, min_depth=0.1):
    """The finite motion's rewrite of tracked points (ofk.h: ofk_finite_correct_points): prev, next [N,2] (or [B,N,2]) pixels as the
    solve would read them, sensors [28] (or [B,28]) the record of the next frame (normal, omega per frame interval, scaling, centre).
    Returns (prev, next) f32 for which solve_lgs' first-order system is the exact relation of the frame pair: its velocity is then
    the displacement per frame interval."""
    return ofk.default_context().finite_correct_points(ofk.finite_motion_setting("exact", min_depth), prev, next, sensors=sensors)


def feasible(x, v, omega, T, u, d, n):
    """node:44-50 (reference not executable: uses v_cr/u_cr before definition, returns nothing).  The evident
    intent — parallelity and distance of each point given the lever-arm corrected velocity — is returned."""
    x = np.asarray(x, np.float64); u = np.asarray(u, np.float64)
    ve = np.asarray(v, np.float64) + np.cross(omega, T)
    v_cross = np.cross(np.concatenate([x[:, :2], np.ones((len(x), 1))], 1), ve[None, :])
    u_cross = np.cross(np.concatenate([x[:, :2], np.zeros((len(x), 1))], 1), np.concatenate([u[:, :2], np.zeros((len(x), 1))], 1))
    vn = np.linalg.norm(v_cross, axis=1); un = np.linalg.norm(u_cross, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        par = np.where(vn * un != 0, np.einsum("ni,ni->n", v_cross, u_cross) / (vn * un), 1.0)
        dist = np.where(un != 0, (np.concatenate([x[:, :2], np.ones((len(x), 1))], 1) @ np.asarray(n, np.float64)) * vn / un / d, 0.0)
    return par, dist


class optical_fusion:
    # parameters the reference sets inline (node:96-107, :182, :241)
    min_feat = 20
    max_feat = 100
    _robust = {}                                                 # PipelineConfig's robust_* settings (see __init__); empty: the plain solve
    _track_gate = {}                                             # PipelineConfig's fb_check / fb_thr / fb_level / err_max; empty: no gate
    _corner_grid = {}                                            # PipelineConfig's grid_cell / grid_cap / grid_max_rank; empty: no grid
    _cov = {}                                                    # PipelineConfig's covariance fields (cov, sigma_*, ...); empty: no covariance
    _joint = {}                                                  # PipelineConfig's joint fields (joint, joint_sigma_flow_px, omega_prior, ...); empty: the gyro is taken as exact
    _gyro_bias = {}                                              # PipelineConfig's gyro_bias field; empty: the gyro is taken as unbiased
    _plane = {}                                                  # PipelineConfig's plane fields (plane, plane_sigma_flow_px, normal_prior, ...); empty: the normal is taken as exact
    _epipolar = {}                                               # PipelineConfig's epipolar fields (epipolar, epi_anchor_px, epi_sigma_max, ...); empty: every depth is the plane's
    _zones = {}                                                  # PipelineConfig's zones / zone_* fields; empty: no exclusion zones
    _camera = {}                                                 # PipelineConfig's camera field; empty: the points are taken as ideal pinhole samples
    _lk_light = {}                                               # PipelineConfig's lk_light field; empty: LK assumes brightness constancy
    _finite_motion = {}                                          # PipelineConfig's finite_motion field; empty: the solve takes the flow as the instantaneous field
    _track_table = {}                                            # PipelineConfig's track_table field; empty: the tracks are anonymous points
    _track_depth = {}                                            # PipelineConfig's track_depth field; empty: no depth per track
    _keyframe_rotation = {}                                      # PipelineConfig's keyframe_rotation field; empty: R_acc is taken as exact
    _pos_filter = {}                                             # PipelineConfig's pos_filter field; empty: no position filter
    _keyframe_map = {}                                           # PipelineConfig's keyframe_map field; empty: the key solve is the plane's
    _stabilise = {}                                              # PipelineConfig's stabilise field; empty: no stabilised view
    _rectify = {}                                                # PipelineConfig's rectify field; empty: the view is not resampled through the lens
    _fix = None                                                  # (position, sigma) of call_fix, handed to the filter with the next frame
    _keyframe = {}                                               # PipelineConfig's keyframe field; empty: no position against a keyframe
    _track_template = {}                                         # PipelineConfig's track_template field; empty: no template per track
    _rolling_shutter = {}                                        # PipelineConfig's rolling_shutter field; empty: every row is taken as exposed at the time stamp
    feature_params = dict(qualityLevel=0.7, minDistance=10, blockSize=12)
    lk_params = dict(winSize=(15, 15), maxLevel=3, criteria=(cv2.TERM_CRITERIA_EPS | cv2.TERM_CRITERIA_COUNT, 20, 0.03))
    scaling = 0.01
    T = 0.0


    # ---- the attributes call_imu owns (node:61-89).  Plain host values while the node runs as shipped; with the restored pipeline
    #      their truth lives on the device between frames and the host copy is refreshed only when somebody reads one
    #      (ofk_imu_state), or pushed down when somebody assigns one.
    def _imu_refresh(self):
        if self._imu_stale and self._stream is not None:
            self._imu_flush()
            st, _ = self._stream.ctx.imu_state(1)
            s0 = st[0]
            d = self._imu
            d["vel"] = s0[0:3].copy(); d["old_time"] = float(s0[3]); d["time_zero"] = int(s0[4]); d["first_imu_"] = bool(s0[5] != 0.0)
            d["rotation"] = s0[6:15].reshape(3, 3).copy(); d["normal"] = s0[15:18].copy(); d["ang"] = s0[18:21].copy(); d["ang_err"] = s0[21:24].copy()
            self._imu_stale = False

    def _imu_flush(self):
        """Host -> device: a state somebody assigned on the host first, then the messages received since the last frame."""
        fs = self._stream
        if fs is None:
            return
        if self._imu_host_dirty:
            d = self._imu
            s0 = np.zeros(ofk.IMU_STATE)
            s0[0:3] = d["vel"]; s0[3] = d["old_time"]; s0[4] = d["time_zero"]; s0[5] = 1.0 if d["first_imu_"] else 0.0
            s0[6:15] = np.asarray(d["rotation"], np.float64).ravel(); s0[15:18] = d["normal"]; s0[18:21] = d["ang"]
            s0[21:24] = np.asarray(d["ang_err"], np.float64).ravel()[:3] if np.size(d["ang_err"]) >= 3 else 0.0
            fs.ctx.imu_reset(1, s0)
            self._imu_host_dirty = False
        if self._imu_pending:
            fs.push_imu(np.stack(self._imu_pending)[None])
            self._imu_pending = []

    def _imu_get(self, name):
        with self._lock:
            self._imu_refresh()
            return self._imu[name]

    def _imu_set(self, name, value):
        with self._lock:
            self._imu_refresh()                                  # messages queued before the assignment are applied before it
            self._imu[name] = value
            if self._stream is not None:
                self._imu_host_dirty = True

    vel = property(lambda self: self._imu_get("vel"), lambda self, v: self._imu_set("vel", v))
    old_time = property(lambda self: self._imu_get("old_time"), lambda self, v: self._imu_set("old_time", v))
    time_zero = property(lambda self: self._imu_get("time_zero"), lambda self, v: self._imu_set("time_zero", v))
    first_imu_ = property(lambda self: self._imu_get("first_imu_"), lambda self, v: self._imu_set("first_imu_", v))
    rotation = property(lambda self: self._imu_get("rotation"), lambda self, v: self._imu_set("rotation", v))
    normal = property(lambda self: self._imu_get("normal"), lambda self, v: self._imu_set("normal", v))
    ang = property(lambda self: self._imu_get("ang"), lambda self, v: self._imu_set("ang", v))
    ang_err = property(lambda self: self._imu_get("ang_err"), lambda self, v: self._imu_set("ang_err", v))

    def call_dist(self, data):
        """node:55-58 — reads the range and discards it (self.d stays 0.75)."""
        distance = data.range  # noqa: F841

    def call_imu(self, data):
        """node:61-89 — quaternion -> R, normal, dead-reckoning between optical fixes (k_imu)."""
        w, q, a, st = data.angular_velocity, data.orientation, data.linear_acceleration, data.header.stamp
        cov = data.angular_velocity_covariance
        msg = np.array([st.secs, st.nsecs, q.x, q.y, q.z, q.w, w.x, w.y, w.z, cov[0], cov[4], cov[8], a.x, a.y, a.z], np.float64)
        with self._lock:
            if self._stream is not None and not self.synthetic_test:
                # The restored pipeline keeps node:61-89's state on the device (FlowStream, FusionConfig.node(): k_imu_seq applies the
                # messages, k_stream_fuse reads normal / omega / R / velocity from there and writes self.vel = v_uav back).  A message
                # costs a list append here; the whole batch since the last frame goes up with that frame (or when an attribute is read).
                self._imu_pending.append(msg)
                self._imu_stale = True
                self.got_ang_vel_ = True
                return
            state = np.zeros(ofk.IMU_STATE)
            state[0:3] = self.vel; state[3] = self.old_time; state[4] = self.time_zero; state[5] = 1.0 if self.first_imu_ else 0.0
            state = self._ctx().imu_propagate(state, msg)
            if not self.got_vel_:                       # node:80 (got_vel_ is never set on self, node:260-262 toggles a local)
                self.vel = state[0:3].copy()
            self.old_time = float(state[3]); self.time_zero = int(state[4]); self.first_imu_ = False
            self.rotation = state[6:15].reshape(3, 3).copy(); self.normal = state[15:18].copy()
            self.ang = state[18:21].copy(); self.ang_err = state[21:24].copy()
            self.got_ang_vel_ = True

    def _decode(self, image_raw):
        """node:112 (cv_bridge.compressed_imgmsg_to_cv2(image_raw, 'bgr8')).  A sensor_msgs/CompressedImage - anything with a
        `.data` byte payload - or a bare JPEG byte string is decoded on the GPU (cv2_hip.imdecode = what cv_bridge calls);
        cv_bridge only takes over for payloads the device decoder does not handle (png, progressive JPEG)."""
        if isinstance(image_raw, np.ndarray):
            return image_raw
        data = image_raw if isinstance(image_raw, (bytes, bytearray, memoryview)) else getattr(image_raw, "data", None)
        if data is not None:
            img = cv2.imdecode(np.frombuffer(bytes(data), np.uint8), cv2.IMREAD_COLOR)
            if img is not None:
                return img
        if CvBridge is None:
            raise RuntimeError("call_optical: not a baseline JPEG payload and cv_bridge is not available - pass BGR numpy frames")
        return CvBridge().compressed_imgmsg_to_cv2(image_raw, 'bgr8')

    def call_optical(self, image_raw):
        """node:92-177 - image callback.  As shipped (synthetic_test) it only decodes, converts and stores the frame; with the
        reference's commented-out pipeline restored the whole frame step runs on the device (_call_optical_resident)."""
        with self._lock:
            if self.got_picture_:
                return
            if not self.synthetic_test:
                return self._call_optical_resident(image_raw)
            image = self._decode(image_raw)
            image_gray = cv2.cvtColor(image, cv2.COLOR_BGR2GRAY)
            if self.first:
                first_feat = np.array([[-401, 300], [399, -300], [400, 301], [-400, -299]])           # node:123
                self.feat = np.asarray(first_feat).reshape((len(first_feat), 2))
                self.feat_err = np.zeros(len(first_feat))
            else:
                self.init = False
                self.got_picture_ = True
            self.old_pic = image_gray
            self.first = False

    def _payload(self, image_raw):
        """The frame as the device wants it: a baseline-JPEG byte string (decoded on the GPU, nothing decoded crosses PCIe) or an
        HxWx3 BGR array.  Anything the device decoder refuses goes through cv_bridge like in the reference (node:112)."""
        if isinstance(image_raw, np.ndarray):
            return image_raw
        data = image_raw if isinstance(image_raw, (bytes, bytearray, memoryview)) else getattr(image_raw, "data", None)
        if data is not None:
            data = bytes(data)
            try:
                h, w, _ = ofk.jpeg_info(data)
                if h <= ofk.MAX_DIM and w <= ofk.MAX_DIM:
                    return data
            except ofk.OfkError:
                pass
        return self._decode(image_raw)

    def _call_optical_resident(self, image_raw):
        """node:112-175 with the commented-out blocks restored, on pipeline.FlowStream: the frame (JPEG or BGR) goes to the device
        once; gray levels, pyramids and the tracks stay in HBM between callbacks.  First frame: goodFeaturesToTrack (:120).  Later
        frames: calcOpticalFlowPyrLK from the resident tracks (:133-136), centre + scale, r_tilde filter with the dead-reckoned
        velocity, solve_lgs, lever arm + rotation (:229-258, the main loop's work, one kernel behind LK), status filter,
        re-detection with a disc mask when <= min_feat tracks are left (:157-166), frame swap (:175).  step() then publishes what
        was computed."""
        frame = self._payload(image_raw)
        is_jpeg = not isinstance(frame, np.ndarray)
        h, w = ofk.jpeg_info(frame)[:2] if is_jpeg else frame.shape[:2]
        if self._stream is None or self._stream_dim != (h, w):
            if self._stream is not None:
                self._stream.close()
            cnt, eps = cv2._criteria(self.lk_params["criteria"])
            cfg = PipelineConfig(max_corners=int(self.max_feat), quality=float(self.feature_params["qualityLevel"]),
                                 min_distance=float(self.feature_params["minDistance"]), block_size=int(self.feature_params["blockSize"]),
                                 win=int(self.lk_params["winSize"][0]), max_level=int(self.lk_params["maxLevel"]), max_count=cnt, eps=eps,
                                 use_feasibility=True, feas_T=float(self.T), **self._robust, **self._track_gate, **self._corner_grid,
                                 **self._cov, **self._joint, **self._plane, **self._epipolar, **self._zones, **self._camera, **self._rolling_shutter,
                                 **self._finite_motion, **self._gyro_bias, **self._lk_light, **self._track_table, **self._track_depth,
                                 **self._track_template, **self._keyframe, **self._keyframe_rotation, **self._pos_filter,
                                 **self._keyframe_map, **self._stabilise, **self._rectify)
            self._stream = FlowStream(w, h, batch=1, cfg=cfg, device=int(os.environ.get("OFK_DEVICE", "0")), min_features=int(self.min_feat),
                                      mask_radius=30, fusion=FusionConfig.node())
            self._stream_dim = (h, w)
            self.first = True
            self._imu_host_dirty = True                          # the dead-reckoning state so far moves to the device with the first step
        fs = self._stream
        if self.first:
            tracks, counts = fs.begin_jpeg([frame]) if is_jpeg else fs.begin(frame[None])
            n = int(counts[0])
            self.feat = tracks[0, :n].astype(np.float64).reshape(n, 2)
            self.feat_err = np.zeros(n)
            self.first = False
            return
        old = np.asarray(self.feat, np.float32).reshape(-1, 2)
        translation = of.pix_trans((320, 240))                   # node:229 (the node centres with (160, 120) whatever the frame size)
        fs._params.feas_T = float(self.T)
        self._imu_flush()                                        # host-side assignments, then the IMU messages since the last frame: one upload
        # normal / omega / R / prior velocity come from the resident IMU state (FusionConfig.node(): use_imu); the record only
        # carries what call_imu does not own
        sc, ccx, ccy = self._camera["camera"].sensor_slots() if self._camera else (self.scaling, translation[0], translation[1])
        sensors = ofk.make_sensors(1, d=self.d, offset=self.offset, scaling=sc, cx=ccx, cy=ccy)
        if self._pos_filter and self._fix is not None:           # call_fix: with this frame's step (a held step keeps it on the device)
            fs.position_input(fix=self._fix[0], fix_sigma=self._fix[1])
            self._fix = None
        rec, fused, tracks, counts = fs.step_fused([frame] if is_jpeg else frame[None], sensors)
        self._imu_stale = True                                   # the step wrote self.vel = v_uav on the device (node:261)
        nxt, keep = fs.ctx.stream_last_points(max(1, len(old)))
        k = keep[0, :len(old)] != 0
        n = int(counts[0])
        self.flow = (nxt[0, :len(old)][k] - old[k]).reshape(-1, 1, 2)                               # node:136
        self.feat = tracks[0, :n].astype(np.float64).reshape(n, 2)                                   # kept points (+ re-detected ones, node:166)
        self.feat_err = np.zeros(n)
        r = rec[0]
        self._resident_result = (r[0:3].copy(), r[8:11].copy(), (np.array([r[3]]) if (r[4] == 3 and 3 * r[11] > 3) else np.empty(0)), int(r[4]),
                                 r[5:8].copy()) if r[15] else None
        if self._cov and r[15]:                                  # the attribute the reference carries and never fills (node:184)
            cv = fs.covariances()[0]
            self.last_cov = cv
            if cv[13] == 0:
                self.vel_err = np.sqrt(np.maximum(cv[[6, 9, 11]], 0.0))
        if self._joint and r[15]:
            self.last_joint = fs.rotations()[0]
        if self._gyro_bias:
            self.last_gyro_bias = fs.gyro_bias()[0]
        if self._plane and r[15]:
            self.last_plane = fs.planes()[0]
        for name, (read, keys) in _LAST_PER_TRACK.items():       # stream 0's entry of every key
            if getattr(self, "_" + name):
                d = read(fs)
                setattr(self, "last_" + name, {k: d[k][0] for k in keys})
        if self._keyframe_map:
            km = fs.key_map()
            self.last_key_map = {k: v[0] for k, v in km.items()}
        if self._stabilise:
            sv = fs.stabilised()
            self.last_stabilised = {k: v[0] for k, v in sv.items()}
        if self._pos_filter:
            fp = fs.fused_position()
            self.last_position = {k: ({n: a[0] for n, a in v.items()} if isinstance(v, dict) else v[0]) for k, v in fp.items()}
        if self._epipolar and r[15]:
            rec, pts = fs.structure()
            self.last_epipolar = (rec[0], pts[0])
        self.init = False
        self.got_picture_ = True

    def call_fix(self, position, sigma):
        """An absolute position fix (GPS, a marker) for the position filter: position [3] in the world frame, sigma a number or [3].
        It is stored and enters the filter with the next frame's step (ofk.h: ofk_pos_filter_input); a later call before that frame
        replaces it.  ValueError without pos_filter, or for a fix or a sigma that is not finite and positive."""
        if not self._pos_filter:
            raise ValueError("call_fix: optical_fusion was built without pos_filter")
        p = np.asarray(position, np.float64).reshape(3)
        s = np.array(np.broadcast_to(np.asarray(sigma, np.float64), (3,)))
        if not (np.isfinite(p).all() and np.isfinite(s).all() and (s > 0).all()):
            raise ValueError(f"call_fix: position {p} must be finite and sigma {s} finite and positive")
        with self._lock:
            self._fix = (p, s)

    def _ctx(self):
        return ofk.default_context()

    def step(self):
        """One pass of the reference's main loop body (node:226-267).  Returns v_obs or None."""
        with self._lock:
            if not (self.got_picture_ and not self.init):
                return None
            if not self.synthetic_test:                          # the callback already ran the loop body on the device (node:229-258)
                res, self._resident_result = self._resident_result, None
                self.got_picture_ = False
                if res is None:
                    return None
                v_obs, v_uav, R, rank, sv = res
                print('    '.join(map(str, v_obs)))                                                          # node:259
                # node:261 self.vel = v_uav happened on the device behind the solve (vel_overwrite); reading self.vel fetches it
                self.last_v_uav = v_uav
                self.last_residual, self.last_rank, self.last_s = R, rank, sv
                return v_obs
            # ---- the node as shipped: 4 test features, flow from generate_test_data, feasibility forced to -1
            translation = of.pix_trans((320, 240))
            x = copy.deepcopy(self.feat).astype(float)
            x[:, 0] = (x[:, 0] - translation[0]) * self.scaling
            x[:, 1] = (x[:, 1] - translation[1]) * self.scaling
            u = generate_test_data(x, np.array([1, 1, 1]), np.array([0, 0, 0]), self.d, np.array([0, 0, 1]))       # node:236
            feasibility, dummy_d = of.r_tilde(x, u, self.normal, self.vel, self.d)                                  # node:238
            feasibility = -1 * np.ones(len(x))                                                                      # node:240
            keep = feasibility <= self.T
            x = x[keep]; u = u[keep]; dummy_d = dummy_d[keep]
            self.feat = self.feat[keep]
            v_obs = None
            if len(x) >= 3:
                v_obs, R, rank, s = solve_lgs(x, u, self.d, self.normal, self.ang)
                v_uav = self._ctx().post_solve(v_obs, self.rotation, self.ang, self.offset)                        # node:258
                if self._cov:
                    self._vel_err_from_solve(x, u)
                print('    '.join(map(str, v_obs)))
                self.vel = v_uav
                self.last_residual, self.last_rank, self.last_s = R, rank, s
            self.got_picture_ = False
            return v_obs

    def _vel_err_from_solve(self, x, u):
        """self.vel_err = sqrt(diag(C_uav)) of the solve just made (the node as shipped solves on the host's points): the stage entry
        with the lever arm, then the rotation, which is taken as exact."""
        c = PipelineConfig(**self._cov)
        setting = ofk.cov_setting(c.cov, c.sigma_flow_px * self.scaling, c.sigma_pos_px * self.scaling, c.sigma_d, c.sigma_omega, c.sigma_normal,
                                  c.sigma_offset)
        _, cv = self._ctx().velocity_solve_cov(ofk.SOLVE_NODE, x[:, :2], u[:, :2], d=float(self.d), nrm=self.normal, omega=self.ang,
                                               t=self.offset, cov=setting)
        self.last_cov = cv
        if cv[13] == 0:
            Rm = np.asarray(self.rotation, np.float64).reshape(3, 3)
            self.vel_err = np.sqrt(np.maximum(np.diag(Rm @ ofk.cov_matrix(cv[6:12]) @ Rm.T), 0.0))

    def __init__(self, spin=True, synthetic_test=True, robust=None, track_gate=None, corner_grid=None, cov=None, zones=None, camera=None,
                 rolling_shutter=None, joint=None, plane=None, finite_motion=None, epipolar=None, gyro_bias=None, lk_light=None,
                 track_table=None, track_depth=None, track_template=None, keyframe=None, keyframe_rotation=None, pos_filter=None,
                 keyframe_map=None, stabilise=None, rectify=None):
        """robust: None (the reference's plain solve) or a dict of PipelineConfig's robust_* settings without the prefix, e.g.
        dict(loss="tukey", hypotheses=64, drop=True): the restored pipeline then solves robustly (ofk.h: ofk_set_robust).
        track_gate: None (every point LK reports as tracked is used) or a dict of ofk.track_gate_setting's keywords, e.g.
        dict(fb="seeded", fb_thr=0.5, fb_level=0): the restored pipeline then drops the points that fail the forward-backward check
        or exceed err_max before the solve and from the tracks (ofk.h: ofk_set_track_gate).
        corner_grid: None (goodFeaturesToTrack's selection) or a dict of ofk.corner_grid_setting's keywords, e.g. dict(cell=64, cap=4):
        detection and re-detection then hold at most `cap` corners per cell, the re-detection counting the tracks that are still
        alive (ofk.h: ofk_set_corner_grid).
        cov: None or a dict of PipelineConfig's covariance fields with `mode` for its `cov`, e.g. dict(mode="propagate",
        sigma_flow_px=0.3, sigma_d=0.05, sigma_omega=0.01): every solved step then fills self.vel_err = sqrt(diag(C_uav)), the
        attribute the reference carries through its callbacks and never reads (ofk.h: ofk_set_cov); self.last_cov is the record.
        zones: None or a dict of ofk.zones_setting's keywords (an empty selection of them: dict(mode="hull")), e.g. dict(link=48,
        radius=20, ttl=30): the points the solve stage rejects build exclusion zones that move with them and keep the re-detection
        off an independently moving object (ofk.h: ofk_set_zones); self._stream.zones() reads the table.
        camera: None (every point is a sample of an ideal pinhole image, centred and scaled with the node's constants) or a
        pipeline.CameraModel (or a dict of its fields), e.g. dict(fx=1000, fy=1010, cx=652.3, cy=470.1, k=(-0.28, 0.09, 0, 0)): the
        restored pipeline then undoes the lens distortion on the device in front of the solve (ofk.h: ofk_set_camera) and takes
        scaling and centre from the model (1 / fo, co_x, co_y) in the place of self.scaling and the node's (160, 120).
        rolling_shutter: None (every row is taken as exposed at the frame's time stamp) or a pipeline.RollingShutter (or a dict of its
        fields), e.g. dict(readout=0.9, mode="gyro", anchor=0.5): the restored pipeline then undoes the per-row capture time on the
        device in front of the solve (ofk.h: ofk_set_rolling_shutter); the node's omega is per frame interval as it stands only if
        omega_gain says so.
        joint: None (the gyro is taken as exact), True, or a dict of sigma_flow_px, omega_prior, omega_prior_from_imu (PipelineConfig's
        joint fields), e.g. dict(sigma_flow_px=0.2, omega_prior=1e-3): every solved step then refines the gyro from the flow and
        reports the joint velocity (ofk.h: ofk_set_joint); self.last_joint is the record, its slots 0-2 the refined omega.
        plane: None (the normal is taken as exact), True, or a dict of sigma_flow_px, normal_prior, sigma_max, range_beam, iters
        (PipelineConfig's plane fields), e.g. dict(normal_prior=0.05): every solved step then refines the ground normal from the flow
        and reports the velocity over the refined plane (ofk.h: ofk_set_plane); self.last_plane is the record, its slots 0-2 the
        refined normal, 3 the refined distance.  Refused beside joint and cov at the first frame.
        epipolar: None (every depth is the plane's), True, or a dict of anchor_px, anchor_min, sigma_max, weights, range_beam
        (PipelineConfig's epipolar fields), e.g. dict(anchor_px=120): every solved step then takes the direction of v from the
        epipolar constraint and its length from the range at the beam's foot (ofk.h: ofk_set_epipolar); self.last_epipolar is
        (record [32], point rows [max_pts, 4]).  Refused beside joint, plane and cov at the first frame.
        finite_motion: None (the flow is taken as the instantaneous motion field), True, an ofk.FiniteMotion or a dict of
        ofk.finite_motion_setting's keywords, e.g. dict(min_depth=0.1): the restored pipeline then writes the frame pair's exact
        rotation and plane displacement into the points on the device in front of the solve (ofk.h: ofk_set_finite_motion); the
        velocity is then the mean over the frame interval, and the node's omega has to be per frame interval.
        gyro_bias: None (the gyro is taken as unbiased), True, an ofk.GyroBias or a dict of ofk.gyro_bias_setting's keywords, e.g.
        dict(sigma_gyro=2e-5, p0=1e-2): the stream then filters the gyro's bias from the flow and takes it out of omega in front of
        every step (ofk.h: ofk_set_gyro_bias); self.last_gyro_bias is the record, its slots 0-2 the bias.
        lk_light: None (LK assumes brightness constancy between the two frames), "bias", "gain", an ofk.LkLight or a dict of
        ofk.lk_light_setting's keywords, e.g. dict(mode="gain", gain_max=4): LK then takes a gain and a bias per window out, which
        is what a camera under auto-exposure needs (ofk.h: ofk_set_lk_light).
        track_table: None (the tracks are anonymous points), True (the table alone), an ofk.TrackTable or a dict of
        ofk.track_table_setting's keywords, e.g. dict(seed="flow"): the stream then keeps an id, an age, a birth and the last flow
        per track on the device, and with seed "flow" starts LK at each track's position plus that flow (ofk.h:
        ofk_set_track_table); self._stream.track_table() reads the table.
        track_depth: None (no depth per track), True, an ofk.TrackDepth or a dict of ofk.track_depth_setting's keywords, e.g.
        dict(q=1e-6): the stream then filters an inverse depth per track on the device and solves a velocity from the depths of the
        earlier frames (ofk.h: ofk_set_track_depth); it switches the track table on when track_table is None.
        self.last_track_depth is dict(rho, var, nobs, ids, rec), rec[0:3] that velocity and rec[3] its flag.
        track_template: None (no template per track), True, an ofk.TrackTemplate or a dict of ofk.track_template_setting's keywords,
        e.g. dict(ncc_min=0.9): the stream then keeps the patch every track was born with, drops the tracks that no longer match it
        and pulls the others back onto it (ofk.h: ofk_set_track_template); it switches the track table on when track_table is None.
        self.last_track_template is dict(A, ncc, flag, tstate, ids, rec).
        keyframe: None (no position against a keyframe), True, an ofk.Keyframe or a dict of ofk.keyframe_setting's keywords, e.g.
        dict(min_share=0.7): the stream then solves its displacement against a held frame and reports a position that does not drift
        with the flow (ofk.h: ofk_set_keyframe); it switches the track table on when track_table is None.  self.last_keyframe is
        FlowStream.position()'s dictionary for the one stream.
        keyframe_rotation: None (R_acc is taken as exact), True, an ofk.KeyframeRotation or a dict of ofk.keyframe_rotation_setting's
        keywords, e.g. dict(sigma_bias=1e-3): the key solve then refines the accumulated rotation with the translation (ofk.h:
        ofk_set_keyframe_rotation); it needs keyframe.  self.last_keyframe_rotation is FlowStream.key_rotation()'s dictionary for the
        one stream.
        pos_filter: None (no position filter), True, an ofk.PosFilter or a dict of ofk.pos_filter_setting's keywords, e.g.
        dict(sigma_v=2e-3, nis_max=16): the stream then fuses the keyframe's displacement, the step's velocity and the fixes of
        call_fix in a filter with a cloned state (ofk.h: ofk_set_pos_filter); it switches the keyframe and the track table on when
        they are None.  self.last_position is FlowStream.fused_position()'s dictionary for the one stream.
        keyframe_map: None (the key solve is the plane's), True, an ofk.KeyframeMap or a dict of ofk.keyframe_map_setting's keywords,
        e.g. dict(rel_max=0.05): the key translation is then solved against the per-track depths frozen at the keyframe (ofk.h:
        ofk_set_keyframe_map); it switches the keyframe, the depths and the track table on when they are None.  self.last_key_map is
        FlowStream.key_map()'s dictionary for the one stream.
        stabilise: None (no stabilised view), True, an ofk.Stabilise or a dict of ofk.stabilise_setting's keywords, e.g.
        dict(mode="rotation", min_cover=0.7): every frame's step then leaves the gray frame warped into the view of the stream's first
        keyframe (ofk.h: ofk_set_stabilise); it switches the keyframe and the track table on when they are None and does not go with a
        rolling shutter, nor with a camera model unless rectify is on.  self.last_stabilised is FlowStream.stabilised()'s dictionary
        for the one stream.
        rectify: None, True, an ofk.Rectify or a dict of ofk.rectify_setting's keywords, e.g. dict(r_max=1.3): with a camera model the
        stabilised view is accepted and every raw frame is warped through the lens's forward map into it (ofk.h: ofk_set_rectify)."""
        self._lock = threading.RLock()
        r = dict(robust or {})
        self._robust = dict(robust=r.pop("loss", "tukey"), **{"robust_" + k: v for k, v in r.items()}) if robust else {}
        g = dict(track_gate or {})
        if g:
            ofk.track_gate_setting(**g)                          # unknown or invalid keywords fail here, not at the first frame
        self._track_gate = dict(fb_check=g.pop("fb", "off"), **g) if track_gate else {}
        k = dict(corner_grid or {})
        if k:
            ofk.corner_grid_setting(**k)                         # unknown or invalid keywords fail here, not at the first frame
        self._corner_grid = {"grid_" + n: v for n, v in k.items()}
        cv = dict(cov or {})
        self._cov = dict(cov=cv.pop("mode", "propagate"), **cv) if cov else {}
        if self._cov:
            PipelineConfig(**self._cov).cov_setting()            # unknown or invalid keywords fail here, not at the first frame
        self.last_cov = None
        if joint:
            j = {} if joint is True else dict(joint)
            if "sigma_flow_px" in j:
                j["joint_sigma_flow_px"] = j.pop("sigma_flow_px")
            self._joint = dict(joint=True, **j)
            PipelineConfig(**self._joint).joint_setting()        # unknown or invalid keywords fail here, not at the first frame
        else:
            self._joint = {}
        self.last_joint = None
        if plane:
            pl = {} if plane is True else dict(plane)
            for short, full in (("sigma_flow_px", "plane_sigma_flow_px"), ("sigma_max", "plane_sigma_max"), ("iters", "plane_iters")):
                if short in pl:
                    pl[full] = pl.pop(short)
            self._plane = dict(plane=True, **pl)
            PipelineConfig(**self._plane).plane_setting()        # unknown or invalid keywords fail here, not at the first frame
        else:
            self._plane = {}
        self.last_plane = None
        if epipolar:
            ep = {} if epipolar is True else dict(epipolar)
            for short in ("anchor_px", "anchor_min", "sigma_max", "weights"):
                if short in ep:
                    ep["epi_" + short] = ep.pop(short)
            self._epipolar = dict(epipolar=True, **ep)
            PipelineConfig(**self._epipolar).epipolar_setting()  # unknown or invalid keywords fail here, not at the first frame
        else:
            self._epipolar = {}
        self.last_epipolar = None
        z = dict(zones or {})
        if zones is not None:
            ofk.zones_setting(**z)                               # unknown or invalid keywords fail here, not at the first frame
        names = dict(link="zone_link", min_members="zone_min", radius="zone_radius", ttl="zone_ttl", max_zones="zone_max")
        self._zones = dict(zones=z.pop("mode", "hull"), **{names[k]: v for k, v in z.items()}) if zones is not None else {}
        if camera is not None:
            cm = camera if isinstance(camera, CameraModel) else CameraModel(**dict(camera))
            cm.setting()                                         # unknown or invalid fields fail here, not at the first frame
            self._camera = dict(camera=cm)
        else:
            self._camera = {}
        if rolling_shutter is not None:
            rs = rolling_shutter if isinstance(rolling_shutter, RollingShutter) else RollingShutter(**dict(rolling_shutter))
            rs.setting()                                         # unknown or invalid fields fail here, not at the first frame
            self._rolling_shutter = dict(rolling_shutter=rs)
        else:
            self._rolling_shutter = {}
        if finite_motion is not None and finite_motion is not False:
            fm = finite_motion if finite_motion is True or isinstance(finite_motion, ofk.FiniteMotion) else ofk.finite_motion_setting(**dict(finite_motion))
            self._finite_motion = dict(finite_motion=fm)
            PipelineConfig(**self._finite_motion).finite_motion_setting()   # invalid fields fail here, not at the first frame
        else:
            self._finite_motion = {}
        if gyro_bias is not None and gyro_bias is not False:
            gb = gyro_bias if gyro_bias is True or isinstance(gyro_bias, ofk.GyroBias) else ofk.gyro_bias_setting(**dict(gyro_bias))
            self._gyro_bias = dict(gyro_bias=gb)
            PipelineConfig(**self._gyro_bias).gyro_bias_setting()    # invalid fields fail here, not at the first frame
        else:
            self._gyro_bias = {}
        self.last_gyro_bias = None
        if lk_light is not None and lk_light is not False:
            lt = ofk.lk_light_setting(**dict(lk_light)) if isinstance(lk_light, dict) else lk_light
            self._lk_light = dict(lk_light=lt)
            PipelineConfig(**self._lk_light).lk_light_setting()      # invalid fields fail here, not at the first frame
        else:
            self._lk_light = {}
        if pos_filter is not None and pos_filter is not False and keyframe is None:
            keyframe = True                                      # the filter fuses the keyframe's displacement
        if stabilise is not None and stabilise is not False and keyframe is None:
            keyframe = True                                      # the view is the keyframe's
        if keyframe_map is not None and keyframe_map is not False:   # the map is the depths', frozen at the keyframe
            keyframe = True if keyframe is None else keyframe
            track_depth = True if track_depth is None else track_depth
        self._rectify = _struct_field("rectify", rectify)
        given = dict(track_table=track_table, track_depth=track_depth, track_template=track_template, keyframe=keyframe,
                     keyframe_rotation=keyframe_rotation, pos_filter=pos_filter, keyframe_map=keyframe_map, stabilise=stabilise)
        for name, value in given.items():                        # the rotation's, the filter's and the map's checks read the keyframe, set in front of them
            beside = self._keyframe if name in ("keyframe_rotation", "pos_filter") else {}
            if name == "stabilise":
                beside = dict(**self._keyframe, **self._camera, **self._rolling_shutter, **self._rectify)
            if name == "keyframe_map":
                beside = dict(**self._keyframe, **self._track_depth, **self._keyframe_rotation)
            setattr(self, "_" + name, _struct_field(name, value, **beside))
        if (self._track_depth or self._track_template or self._keyframe) and not self._track_table:
            self._track_table = dict(track_table=True)           # the three are kept per row of the table
        self.last_track_depth = self.last_track_template = self.last_keyframe = self.last_keyframe_rotation = self.last_position = None
        self.last_key_map = self.last_stabilised = None
        self._fix = None
        self._imu = {}                                           # host copy of the attributes call_imu owns (see the properties above)
        self._imu_pending, self._imu_stale, self._imu_host_dirty = [], False, False
        self._stream = None
        self.synthetic_test = synthetic_test
        self._stream_dim = None                                  # (self._stream: pipeline.FlowStream of the restored pipeline, created with the first frame)
        self._resident_result = None
        self.vel = np.array([0.1, 0.1, 0.1])
        self.vel_err = np.array([0.1, 0.1, 0.1])
        self.feat = np.ones((1, 2))
        self.feat_err = np.ones((1, 1))
        self.flow = np.zeros((1, 1, 2))
        self.flow_err = np.zeros((1, 1, 2))
        self.ang = np.array([0, 0, 0])
        self.ang_err = np.zeros((3, 3))
        self.d = 0.75
        self.d_err = 0
        self.rotation = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]])
        self.old_pic = np.zeros((480, 640))
        self.old_time = 0
        self.time_zero = 0
        self.offset = np.array([0, 0, 0.1])
        self.normal = np.array([0, 0, 1])
        self.normal_err = np.array([0, 0, 1])
        self.init = True
        self.first = True
        self.first_imu_ = True
        self.got_normal_ = False
        self.got_vel_ = False
        self.got_picture_ = False
        self.got_ang_vel_ = False
        if not spin:
            return
        if rospy is None:
            raise RuntimeError("rospy is not installed: construct optical_fusion(spin=False) and drive call_* / step() yourself")
        rospy.Subscriber('/mavros/imu/data', Imu, self.call_imu)
        rospy.Subscriber('/camerav2_1280x960/image_raw/compressed', CompressedImage, self.call_optical)
        rospy.Subscriber('/mavros/distance_sensor/hrlv_ez4_pub', Range, self.call_dist)
        self.visualize = rospy.Publisher('visualisation', Image, queue_size=1)
        while not rospy.is_shutdown():
            if self.step() is None:
                time.sleep(0.0005)          # the reference spins hot; yield the GIL to the callback threads


def main():
    print('++')
    if rospy is None:
        raise SystemExit("velocity_measurment_node needs ROS (rospy, cv_bridge, sensor_msgs)")
    rospy.init_node('velocity_calc')
    print('--')
    try:
        optical_fusion()
    except rospy.ROSInterruptException:
        pass


if __name__ == '__main__':
    main()
