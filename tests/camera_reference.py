"""The camera model of include/ofk.h (ofk_set_camera) restated in numpy: Brown (cv2's pinhole model, rational terms included) and the
equidistant fisheye, undistort and distort, float64 in the header's order with one rounding to float32 at the end, and the fallback
rule.  Plus the experiment that motivates the setting: a velocity solve on points seen through a lens, with and without the model.
Test infrastructure only."""
import numpy as np

from oracle import estimation_oracle as eo

OFF, BROWN, FISHEYE = 0, 1, 2
LIMIT = np.float32(1e6)

# the three lenses of the experiment: (model, coefficients in cv2's order, iterations the experiment's "with the model" column uses)
MILD = (BROWN, (-0.05, 0.01, 0.0, 0.0, 0.0), 5)
STRONG = (BROWN, (-0.28, 0.09, 0.0008, -0.0005, -0.012), 5)
FISH = (FISHEYE, (-0.03, 0.005, -0.001, 0.0002), 10)
FRAME = dict(w=1280, h=960, fx=1000.0, fy=1010.0, cx=652.3, cy=470.1)


def camera(model, k, fx, fy, cx, cy, iters=None, fo_x=None, fo_y=None, co_x=None, co_y=None):
    """A camera as a dict with ofk_camera's fields; k is padded to 8 with zeros; the output matrix defaults to the camera matrix with
    one focal length (fx), which is what ofk_set_camera asks for."""
    kk = np.zeros(8)
    kk[:len(k)] = k
    fo_x = fx if fo_x is None else fo_x
    return dict(model=int(model), iters=int(iters if iters is not None else (20 if model == BROWN else 10)), fx=float(fx), fy=float(fy),
                cx=float(cx), cy=float(cy), k=kk, fo_x=float(fo_x), fo_y=float(fo_x if fo_y is None else fo_y),
                co_x=float(cx if co_x is None else co_x), co_y=float(cy if co_y is None else co_y))


def _theta_poly(cam, th):
    k1, k2, k3, k4 = cam["k"][:4]
    t2 = th * th; t4 = t2 * t2; t6 = t4 * t2; t8 = t4 * t4
    return t2, t4, t6, t8, 1.0 + k1 * t2 + k2 * t4 + k3 * t6 + k4 * t8


def undistort_normalised(cam, x0, y0):
    """(x0, y0) = (pixel - c) / f of the image -> the ideal normalised coordinates, float64, the header's order."""
    x0 = np.asarray(x0, np.float64); y0 = np.asarray(y0, np.float64)
    k = cam["k"]
    with np.errstate(all="ignore"):
        if cam["model"] == BROWN:
            k1, k2, p1, p2, k3, k4, k5, k6 = k
            x, y = x0.copy(), y0.copy()
            for _ in range(cam["iters"]):
                r2 = x * x + y * y
                icd = (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
                dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
                dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
                x = (x0 - dx) * icd
                y = (y0 - dy) * icd
            return x, y
        k1, k2, k3, k4 = k[:4]
        thd = np.sqrt(x0 * x0 + y0 * y0)
        th = thd.copy()
        for _ in range(cam["iters"]):
            t2, t4, t6, t8, poly = _theta_poly(cam, th)
            th = th - (th * poly - thd) / (1.0 + 3.0 * k1 * t2 + 5.0 * k2 * t4 + 7.0 * k3 * t6 + 9.0 * k4 * t8)
        s = np.where(thd < 1e-8, 1.0, np.tan(th) / thd)
        return x0 * s, y0 * s


def distort_normalised(cam, x, y):
    """Ideal normalised coordinates -> (pixel - c) / f of the image: the closed-form forward map."""
    x = np.asarray(x, np.float64); y = np.asarray(y, np.float64)
    k = cam["k"]
    with np.errstate(all="ignore"):
        if cam["model"] == BROWN:
            k1, k2, p1, p2, k3, k4, k5, k6 = k
            r2 = x * x + y * y
            cd = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
            dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            return x * cd + dx, y * cd + dy
        r = np.sqrt(x * x + y * y)
        th = np.arctan(r)
        thd = th * _theta_poly(cam, th)[4]
        s = np.where(r < 1e-8, 1.0, thd / r)
        return x * s, y * s


def _finish(lens_x, lens_y, lin_x, lin_y):
    """One rounding to float32; a point with a coordinate that is not finite or beyond 1e6 takes the linear map (both coordinates)."""
    with np.errstate(all="ignore"):
        ox, oy = lens_x.astype(np.float32), lens_y.astype(np.float32)
        good = (np.abs(ox) <= LIMIT) & (np.abs(oy) <= LIMIT)
        ox = np.where(good, ox, lin_x.astype(np.float32)); oy = np.where(good, oy, lin_y.astype(np.float32))
    return np.stack([ox, oy], -1), good


def undistort_points(cam, pts, full=False):
    """pts [..., 2] float32 image pixels -> float32 ideal pixels (x_u * fo + co)."""
    p = np.asarray(pts, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        x0 = (p[..., 0] - cam["cx"]) / cam["fx"]; y0 = (p[..., 1] - cam["cy"]) / cam["fy"]
        x, y = undistort_normalised(cam, x0, y0)
        out, good = _finish(x * cam["fo_x"] + cam["co_x"], y * cam["fo_y"] + cam["co_y"], x0 * cam["fo_x"] + cam["co_x"], y0 * cam["fo_y"] + cam["co_y"])
    return (out, good) if full else out


def distort_points(cam, pts, full=False):
    """pts [..., 2] float32 ideal pixels -> float32 image pixels."""
    q = np.asarray(pts, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        x = (q[..., 0] - cam["co_x"]) / cam["fo_x"]; y = (q[..., 1] - cam["co_y"]) / cam["fo_y"]
        xd, yd = distort_normalised(cam, x, y)
        out, good = _finish(xd * cam["fx"] + cam["cx"], yd * cam["fy"] + cam["cy"], x * cam["fx"] + cam["cx"], y * cam["fy"] + cam["cy"])
    return (out, good) if full else out


def frame_camera(lens, iters=None, **frame):
    """The experiment's 1280 x 960 camera with one of the lenses above."""
    f = dict(FRAME, **frame)
    model, k, it = lens
    return camera(model, k, f["fx"], f["fy"], f["cx"], f["cy"], iters=it if iters is None else iters)


def round_trip(cam, n=20000, seed=11, w=1280, h=960):
    """undistort -> f32 -> distort -> f32 of n uniform pixels of the frame: (largest distance to the start in pixels, points that took
    the fallback in either direction)."""
    rng = np.random.default_rng(seed)
    px = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], -1).astype(np.float32)
    u, g0 = undistort_points(cam, px, full=True)
    back, g1 = distort_points(cam, u, full=True)
    d = back.astype(np.float64) - px.astype(np.float64)
    return float(np.sqrt((d * d).sum(-1)).max()), int((~g0).sum() + (~g1).sum())


def experiment(lens, iters=None, n=400, seed=7):
    """The velocity solve on points seen through `lens`: ideal points and their model flow are pushed through the lens and rounded to
    f32 pixels; "today" solves with scaling = 1 / fx on the raw pixels, "model" undistorts them (f32 ideal pixels) first.
    -> dict(shift: largest pixel shift of the lens, today, model: relative errors of v)."""
    f = FRAME
    cam = frame_camera(lens, iters)
    v = np.array([0.02, -0.015, 0.004]); om = np.array([0.004, -0.003, 0.01]); d = 1.5
    nrm = np.array([0.05, -0.03, 1.0]); nrm = nrm / np.linalg.norm(nrm)
    rng = np.random.default_rng(seed)
    px = np.stack([rng.uniform(40, f["w"] - 40, n), rng.uniform(40, f["h"] - 40, n)], -1)
    x_next = (px - [f["cx"], f["cy"]]) / [f["fx"], f["fy"]]          # ideal normalised coordinates; the node's solve takes the flow at
    x_prev = x_next - eo.generate_test_data(x_next, v, om, d, nrm)   # the NEW position (node:229-235), so the model flow ends there

    def through_lens(xn):
        xd, yd = distort_normalised(cam, xn[:, 0], xn[:, 1])
        return np.stack([xd * f["fx"] + f["cx"], yd * f["fy"] + f["cy"]], -1).astype(np.float32)

    raw_prev, raw_next = through_lens(x_prev), through_lens(x_next)
    shift = float(np.abs(raw_next.astype(np.float64) - px).max())

    def solve(p_prev, p_next):
        sc = 1.0 / f["fx"]
        pp, pn = p_prev.astype(np.float64), p_next.astype(np.float64)
        x = (pn - [f["cx"], f["cy"]]) * sc; u = (pn - pp) * sc
        got = eo.solve_lgs_node(x, u, d, nrm, om)[0]
        return float(np.linalg.norm(got - v) / np.linalg.norm(v))

    return dict(shift=shift, today=solve(raw_prev, raw_next), model=solve(undistort_points(cam, raw_prev), undistort_points(cam, raw_next)))


def ideal_system(cam, old, new, sr):
    """(x, u, ideal old, ideal new) of the solve stage with the camera on: the ideal pixels, centred and scaled with the sensor row."""
    pu = undistort_points(cam, old).astype(np.float64); nu = undistort_points(cam, new).astype(np.float64)
    return (nu - [sr[20], sr[21]]) * sr[19], (nu - pu) * sr[19], pu, nu


def camera_loop(first_frame, cfg, min_feat, radius, cam, sr, solve, **kw):
    """stream_oracle.NodeLoop of a stream with the camera on: the tracker, the tracks, the zones and the re-detection work on the raw
    pixels as they always did; the solver plug `solve` is handed x and u formed from the ideal pixels of the same points.  sr: the
    stream's sensor row (scaling and centre of the ideal pinhole).  Every step's dict carries ideal = (old, new) as float64."""
    from stream_oracle import NodeLoop, default_lk
    seen = {}
    base = kw.pop("lk", None) or default_lk(cfg)

    def lk(g_prev, g, old):
        new, st, err = base(g_prev, g, old)
        seen["old"] = np.asarray(old, np.float32).reshape(-1, 2); seen["new"] = np.asarray(new, np.float32).reshape(-1, 2)
        return new, st, err

    def ideal_solve(x, u, ok, d, nrm, om):
        ideal = (np.zeros((0, 2)), np.zeros((0, 2)))
        if len(x):
            x, u, pu, nu = ideal_system(cam, seen["old"], seen["new"], sr)
            ideal = (pu, nu)
        return dict(solve(x, u, ok, d, nrm, om), ideal=ideal)

    return NodeLoop(first_frame, cfg, min_feat, radius, lk=lk, solve=ideal_solve, **kw)


# ---- the rendered scene seen through the strong lens (tests/test_camera_reference.py has the figures) and the blow-up cameras
SCENE = dict(h=480, w=640, f=500.0, seed=5, v=(0.02, -0.015, 0.004), omega=(0.004, -0.003, 0.01), d=1.0, max_corners=200)


def blow_up_camera(k1, iters):
    return camera(BROWN, (k1, 0, 0, 0, 0), 1000.0, 1000.0, 0.0, 0.0, iters=iters)


def scene_frames():
    """(frames without a lens, frames through the lens, sensors row, configuration, the camera as the reference's dict)."""
    from of_amd import synth, ofk
    from of_amd.pipeline import CameraModel, PipelineConfig
    s = SCENE
    cm = CameraModel(fx=s["f"], fy=s["f"], cx=s["w"] / 2.0, cy=s["h"] / 2.0, k=STRONG[1])
    kw = dict(v=s["v"], omega=s["omega"], d=s["d"])
    plain = synth.render_pair(s["h"], s["w"], s["seed"], scaling=1.0 / s["f"], **kw)
    lens = synth.render_pair(s["h"], s["w"], s["seed"], camera=cm, **kw)
    assert (lens["scaling"], lens["cx"], lens["cy"]) == (1.0 / s["f"], s["w"] / 2.0, s["h"] / 2.0) == cm.sensor_slots()
    sr = ofk.make_sensors(1, d=s["d"], normal=plain["n"], omega=s["omega"], scaling=1.0 / s["f"], cx=s["w"] / 2.0, cy=s["h"] / 2.0)[0]
    cfg = PipelineConfig(max_corners=s["max_corners"], quality=0.01, min_distance=10, block_size=7)
    return plain, lens, sr, cfg, cm, camera(BROWN, STRONG[1], s["f"], s["f"], s["w"] / 2.0, s["h"] / 2.0)


def solve_ideal(cam, chain, sr):
    """The node solve on the ideal pixels of an oracle chain's tracked points."""
    ok = chain["status"] == 1
    pu = undistort_points(cam, chain["pts"]).astype(np.float64); nu = undistort_points(cam, chain["nxt"]).astype(np.float64)
    x = (nu[ok] - [sr[20], sr[21]]) * sr[19]; u = (nu[ok] - pu[ok]) * sr[19]
    return eo.solve_lgs_node(x, u, sr[0], sr[1:4], sr[4:7])


def rel_err(v):
    t = np.array(SCENE["v"])
    return float(np.linalg.norm(np.asarray(v) - t) / np.linalg.norm(t))
