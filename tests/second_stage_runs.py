"""What the GPU tests of the second-stage solves (joint, plane, epipolar, covariance) share in the resident forms: the stream run of
tests/test_gpu_joint.py with its knobs opened (a setting of any kind, a rangefinder dropout, per-step sensors, other clips, the robust
solve), the pair run beside it, the reference of a step's second-stage record, and the check of a record that carries a flag.
No test file.  The frames, sensors and pipeline configuration are those of tests/test_gpu_joint.py."""
import numpy as np

import epi_reference as er
import joint_reference as jr
import plane_reference as pr
from joint_checks import REC_TOL, RSS_TOL
from point_stage_helpers import bits
from test_plane_reference import TOL as PLANE_TOL

H, W, CORNERS = 120, 160, 64                                     # tests/test_gpu_cov.py's frame
MOTION = dict(v=(0.004, -0.003, 0.002), omega=(0.003, -0.002, 0.004), d=1.0)
GYRO_OFF = np.array([1e-3, -1e-3, 5e-4])
OFFSET = (0.02, -0.01, 0.2)
V_PRIOR = (0.004, -0.003, 0.002)
FUSIONS = ("plain", "ekf6", "node", "replace")
_frames = {}


def pipeline_config(**over):
    from of_amd.pipeline import PipelineConfig
    return PipelineConfig(max_corners=CORNERS, quality=0.01, min_distance=6, block_size=5, win=15, max_level=2, max_count=20, eps=0.03, **over)


def make_fusion(name):
    from of_amd.pipeline import FusionConfig, FilterModel
    if name == "ekf6":
        return FusionConfig.ekf6(r=1e-4, p0=1e-4)
    if name == "node":
        return FusionConfig.node()
    if name == "replace":
        model = FilterModel.kf3()
        model.R = 1e-4 * np.eye(3); model.P0 = 1e-4 * np.eye(3)
        return FusionConfig(filter=True, z_sign=-1.0, z_source=1, redetect_replace=True, model=model)
    return None


def stream_frames(hover=False, motion=MOTION):
    """Two clips of four frames and the renderer's record of them.  hover: stream 1's clip is rendered with v = 0."""
    key = ("stream", hover, tuple(motion["v"]))
    if key not in _frames:
        from of_amd import synth
        seqs = [synth.render_sequence(H, W, 7400 + s, 4, margin=64, **(dict(motion, v=(0.0, 0.0, 0.0)) if hover and s == 1 else motion)) for s in range(2)]
        _frames[key] = (np.stack([s[0] for s in seqs]), seqs[0][1])
    return _frames[key]


def stream_sensors(ofk, info, gyro_off=GYRO_OFF, normals=None):
    sensors = ofk.make_sensors(2, d=info["d"], normal=info["n"], omega=np.asarray(info["omega"]) + gyro_off, offset=OFFSET, scaling=info["scaling"],
                               cx=info["cx"], cy=info["cy"], v_prior=V_PRIOR)
    for s, n in (normals or {}).items():
        sensors[s, 1:4] = n
    return sensors


# kind -> (the context's setter, the download of a FlowStream / FlowPipeline)
KINDS = dict(joint=("set_joint", "rotations"), plane=("set_plane", "planes"), epi=("set_epipolar", "structure"), cov=("set_cov", "covariances"))


def apply_setting(ctx, second):
    if second is not None:
        getattr(ctx, KINDS[second[0]][0])(**second[1])


def download(obj, second):
    return getattr(obj, KINDS[second[0]][1])() if second is not None else None


def stream_run(ofk, second, fusion_name, T=3, drop=None, hover=False, gyro_off=GYRO_OFF, normals=None, robust=None, motion=MOTION):
    """2 streams x T frames; per step what the device reported and what the reference needs.  second: None or (kind, the setting's
    keywords).  drop: the step (1 .. T - 1) at which stream 1's range is NaN.  normals: {stream: the sensors' normal}.  robust: the
    robust loss of the pipeline configuration.  motion: what the clips are rendered with.  Returns the steps, the sensors and the fusion."""
    from of_amd.pipeline import FlowStream
    from stream_oracle import imu_messages
    B = 2
    frames, info = stream_frames(hover, motion)
    cfg = pipeline_config(**(dict(robust=robust, robust_hypotheses=16, robust_iters=3, robust_seed=5) if robust else {}))
    fusion = make_fusion(fusion_name)
    sensors = stream_sensors(ofk, info, gyro_off, normals)
    fs = FlowStream(W, H, batch=B, cfg=cfg, min_features=10, mask_radius=8, fusion=fusion)
    steps = []
    try:
        apply_setting(fs.ctx, second)
        tracks, counts = fs.begin(frames[:, 0])
        rng = np.random.default_rng(31)
        for t in range(1, T):
            imu = dv = None
            if fusion is not None and fusion.use_imu:
                msgs = np.stack([imu_messages(rng, 0.1 * t + 10 * s, 3, rate=np.asarray(info["omega"]) + gyro_off) for s in range(B)])
                fs.push_imu(msgs)
                imu, dv = fs.ctx.imu_state(B)
            sr = sensors
            if drop == t:
                sr = sensors.copy(); sr[1, 0] = np.nan
            old_tracks, old_counts = tracks.copy(), counts.copy()
            if fusion is None:
                rec, tracks, counts = fs.step(frames[:, t], sr)
                fused = x = P = None
            else:
                rec, fused, tracks, counts = fs.step_fused(frames[:, t], sr)
                x, P = fs.ctx.filter_state(B) if fusion.filter else (None, None)
            nxt, keep = fs.ctx.stream_last_points(CORNERS)
            imu_after = fs.ctx.imu_state(B)[0] if fusion is not None and fusion.use_imu else None
            steps.append(dict(rec=rec, fused=fused, old=old_tracks, n=old_counts, nxt=nxt, keep=keep, imu=imu, dv=dv, x=x, P=P, imu_after=imu_after,
                              sr=sr, tracks=tracks.copy(), counts=counts.copy(), second=download(fs, second),
                              weights=fs.ctx.robust_download(B)[0] if robust else None))
    finally:
        fs.close()
    return steps, sensors, fusion


STATE_KEYS = ("rec", "fused", "x", "P", "imu_after", "tracks", "counts", "nxt", "keep")


def assert_same_state(a, b, s, tag):
    """Stream s of two steps: record, fused row, filter, IMU state, tracks, counts, next points and keep flags are the same bits."""
    for k in STATE_KEYS:
        if a[k] is not None:
            assert np.array_equal(bits(a[k][s]), bits(b[k][s])), (tag, k, a[k][s], b[k][s])


def second_of(step, s):
    """Stream s's second-stage record of a step and, for the epipolar solve, its point rows."""
    sec = step["second"]
    return (sec[0][s], sec[1][s]) if isinstance(sec, tuple) else (sec[s], None)


def reference(ofk, second, old, nxt, status, sr, before, keep=None, nrm=None, omega=None, solved=True, w=None):
    """The reference's dict for one problem of a resident form under `second`: before is the record with the setting off."""
    kind, s = second
    kw = dict(keep=keep, nrm=nrm, omega=omega, solved=solved)
    if kind == "joint":
        so = np.broadcast_to(np.asarray(s.get("sigma_omega", np.inf), np.float64), (3,))
        return jr.pair_joint(jr.NODE, old, nxt, status, sr, s["sigma_flow"], tuple(so), before, w=w, **kw)
    if kind == "plane":
        return pr.pair_plane(pr.NODE, old, nxt, status, sr, s["sigma_flow"], s.get("sigma_normal", np.inf), before, sigma_max=s.get("sigma_max", 0.1),
                             beam=s.get("beam", (0.0, 0.0, 1.0)), w=w, **kw)
    assert kind == "epi"
    return er.pair_epi(old, nxt, status, sr, before, anchor_px=s.get("anchor", np.inf), anchor_min=s.get("anchor_min", 5),
                       sigma_max=s.get("sigma_max", ofk.EPI_SIGMA_MAX), beam=s.get("beam", (0.0, 0.0, 1.0)), **kw)


def step_reference(ofk, second, st, s, sensors_row, fusion, before):
    """reference() fed with stream s of a stream step, as tests/test_gpu_joint.py feeds it."""
    n = int(st["n"][s])
    use_imu = fusion is not None and fusion.use_imu
    nrm, om = (st["imu"][s, 15:18], st["imu"][s, 18:21]) if use_imu else (None, None)
    keepf = st["keep"][s, :n].astype(bool) if fusion is not None else None
    w = None if st["weights"] is None or second[0] == "epi" else st["weights"][s, :n]
    return reference(ofk, second, st["old"][s, :n], st["nxt"][s, :n], st["keep"][s, :n], sensors_row, before, keep=keepf, nrm=nrm, omega=om,
                     solved=fusion is None or before[15] != 0, w=w)


def predicted_ratio(ofk, second, ref):
    """The reference's predicted sigma over the setting's gate (inf where S or P H P was singular before a sigma could be formed)."""
    kind, s = second
    if kind == "plane":
        return ref.get("sigma", np.inf) / s.get("sigma_max", 0.1)
    return ref["pred"] / s.get("sigma_max", ofk.EPI_SIGMA_MAX)


def assert_declined(kind, rec, rows, ref, v, rss, tag):
    """A device record that carries a flag against the reference's: the flag, the zeros include/ofk.h names, the record left alone
    (v, rss: fields 0-3 of the record behind the run), and the slots that stay set - copies of inputs to the bit, computed ones within
    REC_TOL of their block's largest entry (the objectives of the plane record within RSS_TOL, as tests/plane_checks.py holds them)."""
    rr = ref["rec"]
    flag = int(ref["flag"])
    assert flag != 0 and rec[10] == flag, (tag, "flag", rec[10], flag)
    assert np.array_equal(bits(np.asarray(v, np.float64)), bits(ref["v"])) and rss == ref["rss"], (tag, "the record is untouched", v, ref["v"])
    assert rec[11] == rr[11] and np.array_equal(bits(rec[6:10]), bits(rr[6:10])), (tag, rec[6:12], rr[6:12])
    if kind == "joint":
        assert np.array_equal(bits(rec[0:3]), bits(rr[0:3])) and not rec[3:6].any() and not rec[15:].any(), (tag, rec)
        if flag == 1:
            assert not rec[12:15].any(), (tag, rec[12:15])
        else:
            assert np.abs(rec[12:15] - rr[12:15]).max() <= REC_TOL * np.abs(rr[12:15]).max(), (tag, rec[12:15], rr[12:15])
    elif kind == "plane":
        assert np.array_equal(bits(rec[0:4]), bits(rr[0:4])) and not rec[4:6].any() and not rec[14:26].any() and not rec[28:].any(), (tag, rec)
        scale = max(np.abs(rr[12:14]).max(), 1e-300)
        assert np.abs(rec[12:14] - rr[12:14]).max() <= REC_TOL * scale, (tag, rec[12:14], rr[12:14])
        floor = 3 * rec[11] * ((PLANE_TOL + 8 * pr.EPS) * ref.get("scale", 0.0)) ** 2
        for k in (26, 27):
            assert abs(rec[k] - rr[k]) <= RSS_TOL * rr[k] + floor, (tag, k, rec[k], rr[k])
    else:
        assert rows is not None and not rows.any(), (tag, "rows of a flagged problem are zero")
        assert rec[3] == 0 and not rec[24:].any(), (tag, rec)
        if flag == 1:
            assert not np.delete(rec, [6, 7, 8, 9, 10, 11]).any(), (tag, rec)
        else:
            if flag == 2:
                assert not rec[18:24].any(), (tag, rec)
            assert np.array_equal(rec[12:14], rr[12:14]), (tag, "anchor and negative counts", rec[12:14], rr[12:14])
            fin = np.isfinite(rr)
            assert np.array_equal(fin, np.isfinite(rec)) and np.array_equal(rec[~fin], rr[~fin]), (tag, rec, rr)
            err = np.abs(rec[fin] - rr[fin]) / er.record_scale(rr)[fin]
            assert err.max() <= REC_TOL, (tag, int(np.flatnonzero(fin)[err.argmax()]), rec, rr)


# ---------------------------------------------------------------------------------------------------- resident pairs
def pair_frames(B, hover=False, motion=MOTION):
    key = ("pairs", hover, tuple(motion["v"]))
    if key not in _frames:
        from of_amd import synth
        prev, nxt, base = synth.make_batch(2, H, W, seed=7300, distinct=2, margin=48, **motion)
        if hover:                                                # pair 1 hovers: the same scene seed's pair with v = 0
            hp, hn, _ = synth.make_batch(2, H, W, seed=7300, distinct=2, margin=48, **dict(motion, v=(0.0, 0.0, 0.0)))
            prev = np.stack([prev[0], hp[1]]); nxt = np.stack([nxt[0], hn[1]])
        _frames[key] = (prev, nxt, base)
    prev, nxt, base = _frames[key]
    idx = np.arange(B) % 2                                       # batch 2 and batch 130 hold the same pairs
    return prev[idx], nxt[idx], base


def pair_sensors(ofk, B, base, normals=None, gyro_off=GYRO_OFF):
    from oracle import estimation_oracle as eo
    p0 = base[0]
    R = eo.quat_to_rot(0.1, -0.05, 0.2, np.sqrt(1 - 0.01 - 0.0025 - 0.04))
    sensors = ofk.make_sensors(B, d=p0["d"], normal=p0["n"], omega=np.asarray(p0["omega"]) + gyro_off, rotation=R, offset=OFFSET,
                               scaling=p0["scaling"], cx=p0["cx"], cy=p0["cy"], v_prior=p0["v"])
    for s, n in (normals or {}).items():
        sensors[s::2, 1:4] = n
    return sensors


def pairs_run(ofk, B, second, slices=1, hover=False, normals=None, gyro_off=GYRO_OFF, motion=MOTION):
    """One pairs run under `second` (None: the setting off) with the resident filter stepped behind it.  Returns the sensors, the run's
    downloads, the second-stage download, and the filter's x and P."""
    from of_amd.pipeline import FlowPipeline, FilterModel
    prev, nxt, base = pair_frames(B, hover, motion)
    sensors = pair_sensors(ofk, B, base, normals, gyro_off)
    model = FilterModel.kf3()
    model.R = 1e-4 * np.eye(3); model.P0 = 1e-4 * np.eye(3)
    pipe = FlowPipeline(W, H, B, pipeline_config(), streams=slices)
    try:
        pipe.ctx.filter_configure(model, B)
        apply_setting(pipe.ctx, second)
        pipe.upload(prev, nxt, sensors)
        out = pipe.run()
        sec = download(pipe, second)
        pipe.ctx.pairs_filter_step(B, z_sign=-1.0, z_source=1)
        x, P = pipe.ctx.filter_state(B)
    finally:
        pipe.close()
    return sensors, out, sec, x, P
