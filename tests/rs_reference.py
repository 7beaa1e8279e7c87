"""The rolling shutter of include/ofk.h (ofk_set_rolling_shutter) restated in numpy: row times, the flow and the gyro correction, float64
in the header's order with one rounding to float32 at the end, and the fallback rule.  Plus the experiment that motivates the setting:
a velocity solve on points each of which was observed at its own row time, with and without the correction.  Test infrastructure only.

The experiment (experiment() below): 400 points over a 1280 x 960 frame, f = 1000, the plane d = 1.5, n ~ (0.05, -0.03, 1) of
tests/camera_reference.py; point paths integrated with RK4 through estimation_oracle.generate_test_data's field, every observation
taken at its own row time (fixed-point iteration on its own row), pixels rounded to f32, estimation_oracle.solve_lgs_node with the
flow at the new position.  Relative deviation of v from the solve of the same motion seen by a global shutter (readout 0), as
readout 0.5 / 0.9 / -0.9:

  motion (per frame)                              anchor  raw points                flow mode                 gyro mode
  SLOW   v (0.02, -0.015, 0.004)                  0.5     0.0087 / 0.0155 / 0.0160  0.0014 / 0.0026 / 0.0027  0.00032 / 0.00059 / 0.00054
         w (0.004, -0.003, 0.01), flow 24 px      0       0.0087 / 0.0155 / 0.0160  0.0027 / 0.0048 / 0.0050  0.00058 / 0.00105 / 0.00100
  FAST   v (0.06, 0.08, 0.004)                    0.5     0.0117 / 0.0213 / 0.0199  0.0037 / 0.0069 / 0.0061  0.00036 / 0.00082 / 0.00022
         w (0.02, -0.03, 0.05), flow 73 px        0       0.0116 / 0.0212 / 0.0201  0.0126 / 0.0231 / 0.0216  0.00064 / 0.00133 / 0.00223
  YAW    v as SLOW                                0.5     0.0954 / 0.1695 / 0.1784  0.0346 / 0.0620 / 0.0644  0.00080 / 0.00152 / 0.00141
         w (0.004, -0.003, 0.15), flow 124 px     0       0.0954 / 0.1695 / 0.1787  0.2938 / 0.5218 / 0.5506  0.00155 / 0.00399 / 0.00284

Raw points sit 4.8 to 91 px from where a global shutter would have seen them, corrected ones 0.01 to 1.8 px (gyro) and 0.03 to
13 px (flow).  Gyro mode stays below 0.25 x the raw deviation in all 18 cases (largest ratio: 0.111, FAST at anchor 0 and readout
-0.9); flow mode with the time stamp at the frame's middle stays below 0.6 x (largest: 0.366, YAW at readout 0.9).  With the time
stamp at the first row, flow mode extrapolates a curved path along a straight line over up to 0.9 frame intervals and no longer helps
on the two fast motions (1.08 x and 3.08 x the raw deviation): recorded, not asserted.
Gyro mode takes the rest of the flow against the exact rotation about the middle of the span (ofk.h).  Against the seed formula's
rotational part at the mid point, (x1 - x0) / span - frot((x0 + x1) / 2), the table's gyro column changes in the fourth digit on SLOW
and FAST and by up to 15 % on YAW (0.00072 / 0.00131 / 0.00157 and 0.00179 / 0.00436 / 0.00359), but a point under pure rotation at
w = (0.02, -0.03, 0.15) then stays 0.1 px from its place where test_rs_reference.py asks for 1e-12.

The rendered scene (scene() below: 480 x 640, f = 500, seed 5, v = (0.01, -0.03, 0.01), w = (0.004, -0.003, 0.004), d = 1,
200 corners, readout 0.9, anchor 0.5, synth.render_pair(rolling_shutter=...) through the C oracle chain), relative error of v:
    the same scene with readout 0         0.0065
    rolling shutter, gyro correction      0.0071   (flow correction: 0.0074)
    rolling shutter, no correction        0.0362
The motion is not camera_reference's (v = (0.02, -0.015, 0.004), w_z = 0.01): there the three figures are 0.0111 / 0.0113 / 0.0241,
the uncorrected error only 2.2 x the baseline's.  Raising w_z does not part them: synth renders the LINEARISED homography, whose own
distance to the flow model grows with w_z squared (w_z = 0.03: 0.082 / 0.089 / 0.107).  A larger vertical translation does: the
rows a point crosses are what a rolling shutter turns into an error.
"""
import numpy as np

from oracle import estimation_oracle as eo

OFF, FLOW, GYRO = 0, 1, 2
LIMIT = np.float32(1e6)


def rshutter(mode, readout, anchor=0.5, rows=960, omega_gain=1.0):
    """A setting as a dict with ofk_rshutter's fields."""
    return dict(mode=int(mode), rows=int(rows), readout=float(readout), anchor=float(anchor), omega_gain=float(omega_gain))


def row_times(rs, raw_prev, raw_next):
    """(t0, t1, span) of the header, float64; raw_* [..., 2]."""
    r0 = np.asarray(raw_prev, np.float64); r1 = np.asarray(raw_next, np.float64)
    H = float(rs["rows"])
    t0 = rs["readout"] * (r0[..., 1] / H - rs["anchor"]); t1 = rs["readout"] * (r1[..., 1] / H - rs["anchor"])
    return t0, t1, 1.0 + (t1 - t0)


def _rotate(x, y, t, om):
    """Rodrigues with phi = -t om on P = (x, y, 1), projected; the header's order."""
    p0 = -t * om[..., 0]; p1 = -t * om[..., 1]; p2 = -t * om[..., 2]
    th2 = p0 * p0 + p1 * p1 + p2 * p2
    small = th2 < 1e-16
    th = np.sqrt(np.where(small, 1.0, th2))
    A = np.where(small, 1.0, np.sin(th) / th)
    B = np.where(small, 0.5, (1.0 - np.cos(th)) / np.where(small, 1.0, th2))
    c0 = p1 - p2 * y; c1 = p2 * x - p0; c2 = p0 * y - p1 * x
    d0 = p1 * c2 - p2 * c1; d1 = p2 * c0 - p0 * c2; d2 = p0 * c1 - p1 * c0
    X = x + A * c0 + B * d0; Y = y + A * c1 + B * d1; Z = 1.0 + A * c2 + B * d2
    return X / Z, Y / Z


def correct_f64(rs, raw_prev, raw_next, ideal_prev=None, ideal_next=None, sensors=None):
    """The header's arithmetic before the rounding: (out_prev, out_next, span, usable) in float64; q = ideal_* or the raw points;
    sensors [..., 28] broadcast against the points' leading axes (gyro mode).  usable: scaling != 0 (gyro)."""
    q0 = np.asarray(raw_prev if ideal_prev is None else ideal_prev, np.float64)
    q1 = np.asarray(raw_next if ideal_next is None else ideal_next, np.float64)
    with np.errstate(all="ignore"):
        t0, t1, span = row_times(rs, raw_prev, raw_next)
        if rs["mode"] == FLOW:
            f = (q1 - q0) / span[..., None]
            return q0 - t0[..., None] * f, q1 - t1[..., None] * f, span, np.ones(span.shape, bool)
        sn = np.asarray(sensors, np.float64)
        sc = sn[..., 19]; c = sn[..., 20:22]
        om = rs["omega_gain"] * sn[..., 4:7]
        x0 = (q0[..., 0] - c[..., 0]) * sc; y0 = (q0[..., 1] - c[..., 1]) * sc
        x1 = (q1[..., 0] - c[..., 0]) * sc; y1 = (q1[..., 1] - c[..., 1]) * sc
        hs = span / 2.0
        rx, ry = _rotate(x0, y0, -hs, om); sx, sy = _rotate(x1, y1, hs, om)
        ftx = (sx - rx) / span; fty = (sy - ry) / span
        ax, ay = _rotate(x0, y0, t0, om); bx, by = _rotate(x1, y1, t1, om)
        o0 = np.stack([(ax - t0 * ftx) / sc + c[..., 0], (ay - t0 * fty) / sc + c[..., 1]], -1)
        o1 = np.stack([(bx - t1 * ftx) / sc + c[..., 0], (by - t1 * fty) / sc + c[..., 1]], -1)
        return o0, o1, span, np.broadcast_to(sc != 0.0, span.shape)


def correct_points(rs, raw_prev, raw_next, ideal_prev=None, ideal_next=None, sensors=None, full=False):
    """float32 points [B, S, 2] (or [S, 2]) -> the float32 pair the device writes; sensors [B, 28] (one row per image)."""
    rp = np.asarray(raw_prev, np.float32); rn = np.asarray(raw_next, np.float32)
    q0 = rp if ideal_prev is None else np.asarray(ideal_prev, np.float32)
    q1 = rn if ideal_next is None else np.asarray(ideal_next, np.float32)
    sn = None
    if sensors is not None:
        sn = np.asarray(sensors, np.float64)
        sn = sn[:, None, :] if rp.ndim == 3 else sn.reshape(1, -1)
    with np.errstate(all="ignore"):
        o0, o1, span, usable = correct_f64(rs, rp, rn, q0, q1, sn)
        a, b = o0.astype(np.float32), o1.astype(np.float32)
        good = usable & np.isfinite(span) & (span >= 0.5) & (np.abs(a) <= LIMIT).all(-1) & (np.abs(b) <= LIMIT).all(-1)
    a = np.where(good[..., None], a, q0); b = np.where(good[..., None], b, q1)
    return (a, b, good) if full else (a, b)


# ---------------------------------------------------------------------------------------------------- the experiment
FRAME = dict(w=1280, h=960, f=1000.0, cx=640.0, cy=480.0)
PLANE = dict(d=1.5, n=np.array([0.05, -0.03, 1.0]) / np.linalg.norm([0.05, -0.03, 1.0]))
SLOW = dict(v=(0.02, -0.015, 0.004), omega=(0.004, -0.003, 0.01))
FAST = dict(v=(0.06, 0.08, 0.004), omega=(0.02, -0.03, 0.05))
YAW = dict(v=(0.02, -0.015, 0.004), omega=(0.004, -0.003, 0.15))
MOTIONS = dict(slow=SLOW, fast=FAST, yaw=YAW)
READOUTS = (0.5, 0.9, -0.9)
ANCHORS = (0.5, 0.0)


def advance(x, t, motion, steps=24):
    """Points x [N, 2] (ideal normalised) carried over the times t [N] (either sign) through the flow field: RK4, `steps` steps each."""
    v, om = np.array(motion["v"]), np.array(motion["omega"])
    f = lambda p: eo.generate_test_data(p, v, om, PLANE["d"], PLANE["n"])
    h = (np.asarray(t, np.float64) / steps)[:, None]
    x = np.array(x, np.float64)
    for _ in range(steps):
        k1 = f(x); k2 = f(x + 0.5 * h * k1); k3 = f(x + 0.5 * h * k2); k4 = f(x + h * k3)
        x = x + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return x


def observe(x_stamp, motion, readout, anchor):
    """Where a rolling shutter sees the points that stand at x_stamp at the frame's time stamp: each at its own row time t =
    readout * (row / H - anchor), found by fixed-point iteration on its own row.  -> (f32 pixels, t)."""
    F = FRAME
    t = np.zeros(len(x_stamp))
    for _ in range(12):
        x = advance(x_stamp, t, motion)
        t = readout * ((x[:, 1] * F["f"] + F["cy"]) / F["h"] - anchor)
    x = advance(x_stamp, t, motion)
    return np.stack([x[:, 0] * F["f"] + F["cx"], x[:, 1] * F["f"] + F["cy"]], -1).astype(np.float32), t


def sensor_row(motion, scaling, cx, cy, d=None, n=None):
    sr = np.zeros(28)
    sr[0] = PLANE["d"] if d is None else d
    sr[1:4] = PLANE["n"] if n is None else n
    sr[4:7] = motion["omega"]
    sr[7:16] = np.eye(3).ravel()
    sr[19:22] = scaling, cx, cy
    return sr


def solve_points(p_prev, p_next, sr):
    pp, pn = np.asarray(p_prev, np.float64), np.asarray(p_next, np.float64)
    x = (pn - sr[20:22]) * sr[19]; u = (pn - pp) * sr[19]
    return eo.solve_lgs_node(x, u, sr[0], sr[1:4], sr[4:7])[0]


def experiment(motion, readout, anchor, n=400, seed=7):
    """-> dict(flow_px: the largest flow; shift_px: how far the raw points sit from the global shutter's; raw, flow, gyro: relative
    deviations of v from the global shutter's solve; flow_px_off / gyro_px_off: how far the corrected points sit from it)."""
    F = FRAME
    rng = np.random.default_rng(seed)
    px = np.stack([rng.uniform(40, F["w"] - 40, n), rng.uniform(40, F["h"] - 40, n)], -1)
    x_next = (px - [F["cx"], F["cy"]]) / F["f"]                  # the node's solve takes the flow at the NEW position
    x_prev = advance(x_next, -np.ones(n), motion)
    to_px = lambda x: np.stack([x[:, 0] * F["f"] + F["cx"], x[:, 1] * F["f"] + F["cy"]], -1).astype(np.float32)
    gs_prev, gs_next = to_px(x_prev), to_px(x_next)
    raw_prev, _ = observe(x_prev, motion, readout, anchor)
    raw_next, _ = observe(x_next, motion, readout, anchor)
    sr = sensor_row(motion, 1.0 / F["f"], F["cx"], F["cy"])
    v_gs = solve_points(gs_prev, gs_next, sr)
    dev = lambda a, b: float(np.linalg.norm(solve_points(a, b, sr) - v_gs) / np.linalg.norm(v_gs))
    off = lambda a, b: float(max(np.abs(a.astype(np.float64) - gs_prev).max(), np.abs(b.astype(np.float64) - gs_next).max()))
    out = dict(flow_px=float(np.sqrt(((gs_next.astype(np.float64) - gs_prev) ** 2).sum(-1)).max()), shift_px=off(raw_prev, raw_next),
               raw=dev(raw_prev, raw_next))
    for name, mode in (("flow", FLOW), ("gyro", GYRO)):
        a, b, good = correct_points(rshutter(mode, readout, anchor, F["h"]), raw_prev, raw_next, sensors=sr[None], full=True)
        assert good.all()
        out[name] = dev(a, b); out[name + "_px_off"] = off(a, b)
    return out


def rs_loop(first_frame, cfg, min_feat, radius, rs, sr, solve, given=None, **kw):
    """stream_oracle.NodeLoop of a stream with the rolling shutter on: the tracker, the tracks, the zones and the re-detection work on
    the raw pixels as they always did; the solver plug `solve` is handed x and u formed from the corrected points of the same points.
    sr: the stream's sensor row.  given: a dict whose "pts" = (prev, next) [>= n, 2] f32, when set, are the corrected points the
    solver takes in the place of the restatement's own (the device's, which may differ from them by one ulp in gyro mode).  Every
    step's dict carries ideal = the restatement's (prev, next) as f32."""
    from stream_oracle import NodeLoop, default_lk
    seen = {}
    base = kw.pop("lk", None) or default_lk(cfg)

    def lk(g_prev, g, old):
        new, st, err = base(g_prev, g, old)
        seen["old"] = np.asarray(old, np.float32).reshape(-1, 2); seen["new"] = np.asarray(new, np.float32).reshape(-1, 2)
        return new, st, err

    def corrected_solve(x, u, ok, d, nrm, om):
        ideal = (np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))
        if len(x):
            ideal = correct_points(rs, seen["old"], seen["new"], sensors=sr[None])
            pu, nu = ideal if not (given or {}).get("pts") else [np.asarray(a[:len(x)], np.float64) for a in given["pts"]]
            pu = np.asarray(pu, np.float64); nu = np.asarray(nu, np.float64)
            x = (nu - sr[20:22]) * sr[19]; u = (nu - pu) * sr[19]
        return dict(solve(x, u, ok, d, nrm, om), ideal=ideal)

    return NodeLoop(first_frame, cfg, min_feat, radius, lk=lk, solve=corrected_solve, **kw)


# ---------------------------------------------------------------------------------------------------- the rendered scene
SCENE = dict(h=480, w=640, f=500.0, seed=5, v=(0.01, -0.03, 0.01), omega=(0.004, -0.003, 0.004), d=1.0, max_corners=200, readout=0.9, anchor=0.5)


def scene(readout=None):
    """(frames, sensors row, configuration, the setting as the reference's dict) of the scene rendered with `readout` (None: SCENE's)."""
    from of_amd import synth, ofk
    from of_amd.pipeline import PipelineConfig, RollingShutter
    s = SCENE
    ro = s["readout"] if readout is None else readout
    fr = synth.render_pair(s["h"], s["w"], s["seed"], v=s["v"], omega=s["omega"], d=s["d"], scaling=1.0 / s["f"],
                           rolling_shutter=RollingShutter(readout=ro, mode="gyro", anchor=s["anchor"]))
    sr = ofk.make_sensors(1, d=s["d"], normal=fr["n"], omega=s["omega"], scaling=1.0 / s["f"], cx=s["w"] / 2.0, cy=s["h"] / 2.0)[0]
    cfg = PipelineConfig(max_corners=s["max_corners"], quality=0.01, min_distance=10, block_size=7)
    return fr, sr, cfg, rshutter(GYRO, ro, s["anchor"], s["h"])


def solve_corrected(rs, chain, sr):
    """The node solve on the corrected points of an oracle chain's tracked points."""
    ok = chain["status"] == 1
    a, b = correct_points(rs, chain["pts"], chain["nxt"], sensors=sr[None])
    return solve_points(a[ok], b[ok], sr)


def rel_err(v):
    t = np.array(SCENE["v"])
    return float(np.linalg.norm(np.asarray(v) - t) / np.linalg.norm(t))
