"""The finite motion of include/ofk.h (ofk_set_finite_motion) restated in numpy: the same arithmetic in the same order, the same
thresholds and the same single rounding to float32, and an exact scene generator to hold it against.

A frame pair is the rigid motion P1 = R P0 + T, R = exp([omega]x); the solves build the instantaneous field.  For points on the plane
n.P1 = d (n, d in the NEXT frame's axes):  R P0 = (I - T n' / d) P1, so with q~ = R p0 renormalised and p1 the next point
    (n.p1) / d [q~]x T = [q~]x (p1 - q~),
and the pair x^ = q~, u^ = s (p1 - q~) + rotfield(q~, omega), s = (n.q~) / (n.p1), makes the NODE / SIM systems that relation.

What the plain solve loses and the rewrite gives back (tests/test_finite_reference.py prints it; 400 exact plane points in a
+-0.6 x +-0.45 field, n tilted 3 degrees, d = 1, focal length 800 px, seed 11; |v - T| / |T|, for row 5 |v|):
    T per frame             omega per frame        largest flow   plain     rewritten, f64   rewritten, f32 pixels
    (0.003, -0.002, 0.001)  (0.002, -0.001, 0.003)   5 px         0.0030    3.1e-14          1.4e-6
    (0.03, -0.02, 0.01)     (0.01, -0.02, 0.03)     42 px         0.0291    2.0e-15          2.8e-8
    (0.06, 0.03, -0.02)     (0.02, 0.03, 0.08)     128 px         0.0997    3.7e-16          6.0e-8
    (0.05, -0.04, 0.03)     (0.05, -0.04, 0.15)    156 px         0.1833    8.6e-16          1.6e-8
    0                       (0.03, -0.02, 0.15)    115 px         0.0106    4.6e-17          3.5e-9     (|v|: the false velocity per frame)
The proposal's figures for the plain column (MOTIONS below: another draw of the points) were 0.0031, 0.029, 0.102, 0.185, 0.0108.
"""
import numpy as np

from oracle import estimation_oracle as eo

OFF, EXACT = 0, 1
LIMIT = np.float32(1e6)
DEN_MIN = 1e-12

# the five motions: (T, omega) per frame, and the figures the plain solve was measured at (relative error; row 5: |v|)
MOTIONS = (
    dict(T=(0.003, -0.002, 0.001), omega=(0.002, -0.001, 0.003), flow_px=5.0, plain=0.0031),
    dict(T=(0.03, -0.02, 0.01), omega=(0.01, -0.02, 0.03), flow_px=39.0, plain=0.029),
    dict(T=(0.06, 0.03, -0.02), omega=(0.02, 0.03, 0.08), flow_px=128.0, plain=0.102),
    dict(T=(0.05, -0.04, 0.03), omega=(0.05, -0.04, 0.15), flow_px=149.0, plain=0.185),
    dict(T=(0.0, 0.0, 0.0), omega=(0.03, -0.02, 0.15), flow_px=99.0, plain=0.0108),
)
FOCAL, CENTRE, FIELD, TILT_DEG, N_POINTS = 800.0, (640.0, 480.0), (0.6, 0.45), 3.0, 400


def setting(mode=EXACT, min_depth=0.1):
    """A setting as a dict with ofk_finite_motion's fields."""
    return dict(mode=int(mode), min_depth=float(min_depth))


def rotate3(x, y, om):
    """Rodrigues with phi = +om on P = (x, y, 1), not projected: the rolling shutter's rot() at t = -1, in the header's order."""
    p0 = -(-1.0) * om[..., 0]; p1 = -(-1.0) * om[..., 1]; p2 = -(-1.0) * om[..., 2]
    th2 = p0 * p0 + p1 * p1 + p2 * p2
    small = th2 < 1e-16
    th = np.sqrt(np.where(small, 1.0, th2))
    A = np.where(small, 1.0, np.sin(th) / th)
    B = np.where(small, 0.5, (1.0 - np.cos(th)) / np.where(small, 1.0, th2))
    c0 = p1 - p2 * y; c1 = p2 * x - p0; c2 = p0 * y - p1 * x
    d0 = p1 * c2 - p2 * c1; d1 = p2 * c0 - p0 * c2; d2 = p0 * c1 - p1 * c0
    return x + A * c0 + B * d0, y + A * c1 + B * d1, 1.0 + A * c2 + B * d2


def correct_f64(fm, prev, nxt, sensors, normal=None, omega=None):
    """The header's arithmetic before the rounding: (out_prev, out_next, good) in float64.  prev, nxt [..., 2]; sensors [..., 28]
    broadcast against the points' leading axes; normal / omega: the resident IMU state's in the place of sensors[1..3] / [4..6].
    good: none of the fallback conditions that can be told before the rounding holds."""
    q0 = np.asarray(prev, np.float64); q1 = np.asarray(nxt, np.float64)
    sn = np.asarray(sensors, np.float64)
    with np.errstate(all="ignore"):
        sc = sn[..., 19]; cx = sn[..., 20]; cy = sn[..., 21]
        n = sn[..., 1:4] if normal is None else np.asarray(normal, np.float64)
        om = sn[..., 4:7] if omega is None else np.asarray(omega, np.float64)
        x0 = (q0[..., 0] - cx) * sc; y0 = (q0[..., 1] - cy) * sc
        x1 = (q1[..., 0] - cx) * sc; y1 = (q1[..., 1] - cy) * sc
        X, Y, Z = rotate3(x0, y0, om)
        a = X / Z; b = Y / Z
        den = n[..., 0] * x1 + n[..., 1] * y1 + n[..., 2]
        s = (n[..., 0] * a + n[..., 1] * b + n[..., 2]) / den
        c0 = om[..., 1] - om[..., 2] * b; c1 = om[..., 2] * a - om[..., 0]; c2 = om[..., 0] * b - om[..., 1] * a
        ux = s * (x1 - a) + (c0 - c2 * a); uy = s * (y1 - b) + (c1 - c2 * b)
        o1 = np.stack([a / sc + cx, b / sc + cy], -1)
        o0 = np.stack([(a - ux) / sc + cx, (b - uy) / sc + cy], -1)
        good = (sc != 0.0) & (Z >= fm["min_depth"]) & (np.abs(den) >= DEN_MIN) & (s > 0.0)
        good = np.broadcast_to(good, o0.shape[:-1])
    return o0, o1, good


def correct_points(fm, prev, nxt, sensors, normal=None, omega=None, full=False):
    """float32 points [B, S, 2] (or [S, 2]) -> the float32 pair the device writes; sensors [B, 28] (one row per image), normal /
    omega [B, 3] where the IMU state supplies them."""
    q0 = np.asarray(prev, np.float32); q1 = np.asarray(nxt, np.float32)
    sn = np.asarray(sensors, np.float64)
    per_image = q0.ndim == 3
    sn = sn[:, None, :] if per_image else sn.reshape(1, -1)
    if normal is not None:
        normal = np.asarray(normal, np.float64)
        normal = normal[:, None, :] if per_image else normal.reshape(1, 3)
    if omega is not None:
        omega = np.asarray(omega, np.float64)
        omega = omega[:, None, :] if per_image else omega.reshape(1, 3)
    with np.errstate(all="ignore"):
        o0, o1, good = correct_f64(fm, q0, q1, sn, normal, omega)
        a, b = o0.astype(np.float32), o1.astype(np.float32)
        good = good & (np.abs(a) <= LIMIT).all(-1) & (np.abs(b) <= LIMIT).all(-1)      # false for NaN and infinity too
    a = np.where(good[..., None], a, q0); b = np.where(good[..., None], b, q1)
    return (a, b, good) if full else (a, b)


# ---------------------------------------------------------------------------------------------------- the exact scene
def rotation(omega):
    """exp([omega]x), Rodrigues."""
    om = np.asarray(omega, np.float64)
    W = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    th = np.linalg.norm(om)
    if th < 1e-12:
        return np.eye(3) + W
    return np.eye(3) + (np.sin(th) / th) * W + ((1.0 - np.cos(th)) / th ** 2) * (W @ W)


def tilted_normal(deg=TILT_DEG):
    t = np.deg2rad(deg)
    n = np.array([np.sin(t) * np.cos(0.7), np.sin(t) * np.sin(0.7), np.cos(t)])
    return n / np.linalg.norm(n)


def exact_scene(T, omega, n=N_POINTS, seed=11, d0=None, d1=1.0, n1=None, field=FIELD):
    """Points on a plane seen before and after P1 = R P0 + T.  The plane is given in the NEXT frame's axes (n1, d1: what the sensor
    record carries), so n0 = R' n1 and d0 = d1 - n1.T; with d0 given instead, d1 = d0 + n1.T.  The previous frame's points are drawn
    uniformly in the field.  -> dict(x0, x1 [n, 2] normalised, n0, d0, n1, d1, R, T, omega)."""
    T = np.asarray(T, np.float64); omega = np.asarray(omega, np.float64)
    R = rotation(omega)
    n1 = tilted_normal() if n1 is None else np.asarray(n1, np.float64)
    if d0 is not None:
        d1 = float(d0) + float(n1 @ T)
    n0 = R.T @ n1; d0 = float(d1) - float(n1 @ T)
    rng = np.random.default_rng(seed)
    x0 = np.stack([rng.uniform(-field[0], field[0], n), rng.uniform(-field[1], field[1], n)], -1)
    p0 = np.concatenate([x0, np.ones((n, 1))], 1)
    P0 = p0 * (d0 / (p0 @ n0))[:, None]                          # n0.P0 = d0
    P1 = P0 @ R.T + T
    assert np.allclose(P1 @ n1, d1, rtol=0, atol=1e-12)
    return dict(x0=x0, x1=P1[:, :2] / P1[:, 2:3], n0=n0, d0=d0, n1=n1, d1=float(d1), R=R, T=T, omega=omega)


def sensor_row(sc, scaling=1.0 / FOCAL, cx=CENTRE[0], cy=CENTRE[1]):
    """The record of the next frame of an exact scene."""
    sr = np.zeros(28)
    sr[0] = sc["d1"]; sr[1:4] = sc["n1"]; sr[4:7] = sc["omega"]
    sr[7:16] = np.eye(3).ravel()
    sr[19:22] = scaling, cx, cy
    return sr


def to_px(x, sr):
    return np.asarray(x, np.float64) / sr[19] + sr[20:22]


def xu(p_prev, p_next, sr):
    """What every solve forms from its two point sets: x at the NEW position, u = new - old."""
    pp, pn = np.asarray(p_prev, np.float64), np.asarray(p_next, np.float64)
    return (pn - sr[20:22]) * sr[19], (pn - pp) * sr[19]


def solve_points(p_prev, p_next, sr, variant="node"):
    x, u = xu(p_prev, p_next, sr)
    if variant == "sim":
        return eo.solve_lgs_sim(x, u, sr[0], sr[1:4], sr[4:7], np.zeros(3))[0]
    return eo.solve_lgs_node(x, u, sr[0], sr[1:4], sr[4:7])[0]


def error(v, T):
    """|v - T| / |T|, or |v| where T = 0."""
    T = np.asarray(T, np.float64)
    nt = np.linalg.norm(T)
    return float(np.linalg.norm(np.asarray(v) - T) / nt) if nt > 0 else float(np.linalg.norm(v))


def max_flow_px(sc, sr):
    return float(np.sqrt((((sc["x1"] - sc["x0"]) / sr[19]) ** 2).sum(-1)).max())


def finite_loop(first_frame, cfg, min_feat, radius, fm, sr, solve, given=None, **kw):
    """stream_oracle.NodeLoop of a stream with the finite motion on: the tracker, the tracks, the zones and the re-detection work on the
    raw pixels as they always did; the solver plug `solve` is handed x and u formed from the rewritten points of the same points.
    sr: the stream's sensor row (given["sr"], when set, is the step's own: the resident IMU state's normal and omega written into it).
    given["pts"] = (prev, next) [>= n, 2] f32, when set, are the rewritten points the solver takes in the place of the restatement's own
    (the device's, which may differ from them by one ulp).  Every step's dict carries ideal = the restatement's (prev, next) as f32."""
    from stream_oracle import NodeLoop, default_lk
    seen = {}
    base = kw.pop("lk", None) or default_lk(cfg)

    def lk(g_prev, g, old):
        new, st, err = base(g_prev, g, old)
        seen["old"] = np.asarray(old, np.float32).reshape(-1, 2); seen["new"] = np.asarray(new, np.float32).reshape(-1, 2)
        return new, st, err

    def rewritten_solve(x, u, ok, d, nrm, om):
        ideal = (np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))
        if len(x):
            row = (given or {}).get("sr", sr)
            ideal = correct_points(fm, seen["old"], seen["new"], row[None])
            pu, nu = ideal if not (given or {}).get("pts") else [np.asarray(a[:len(x)], np.float64) for a in given["pts"]]
            pu = np.asarray(pu, np.float64); nu = np.asarray(nu, np.float64)
            x = (nu - row[20:22]) * row[19]; u = (nu - pu) * row[19]
        return dict(solve(x, u, ok, d, nrm, om), ideal=ideal)

    return NodeLoop(first_frame, cfg, min_feat, radius, lk=lk, solve=rewritten_solve, **kw)


# ---------------------------------------------------------------------------------------------------- the rendered scene
SCENE = dict(h=480, w=640, f=800.0, seed=5, T=MOTIONS[1]["T"], omega=MOTIONS[1]["omega"], d=1.0, max_corners=200)


def scene():
    """(frames, sensors row, configuration) of the pair rendered with motion="finite" at row 2's motion.  LK is seeded from the sensor
    model (ofk_set_lk_seed): unseeded, a 15 x 15 window on four levels loses most of the points at 42 px of flow, and what the solve
    then shows is the tracker's error, with the setting on or off."""
    from of_amd import synth, ofk
    from of_amd.pipeline import PipelineConfig
    s = SCENE
    fr = synth.render_pair(s["h"], s["w"], s["seed"], v=s["T"], omega=s["omega"], d=s["d"], n=tilted_normal(), scaling=1.0 / s["f"],
                           margin=96, motion="finite")
    sr = ofk.make_sensors(1, d=s["d"], normal=fr["n"], omega=s["omega"], scaling=1.0 / s["f"], cx=s["w"] / 2.0, cy=s["h"] / 2.0, v_prior=s["T"])[0]
    cfg = PipelineConfig(max_corners=s["max_corners"], quality=0.01, min_distance=10, block_size=7, max_level=3, lk_seed="model", seed_gain=1.0)
    return fr, sr, cfg
