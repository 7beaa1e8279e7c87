"""synth.py — synthetic frame-pair renderer (measurement harness; numpy only).

The reference never synthesises images (numerical_simulation/simulation.py generates point flows,
its videos are missing blobs), so every benchmark/test frame comes from here: a seeded, band-limited
texture on the ground plane, viewed before and after the plane-induced homography
    p2 ~ (I + [w]x + v n^T / d) p1
whose first-order displacement is exactly the reference's flow model (node:25-29; simulation.py:7-12).
v and w are per-frame quantities (velocity*dt, rate*dt), p in normalised centred coordinates
x = (px - c) * scaling (node:229-235).
"""
import numpy as np


def _blur(a, sigma):
    r = max(1, int(3 * sigma + 0.5))
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2); k /= k.sum()
    for axis in (0, 1):
        pad = [(r, r) if ax == axis else (0, 0) for ax in range(2)]
        ap = np.pad(a, pad, mode="reflect")
        out = np.zeros_like(a)
        for i, kv in enumerate(k):
            sl = [slice(None)] * 2
            sl[axis] = slice(i, i + a.shape[axis])
            out += kv * ap[tuple(sl)]
        a = out
    return a


def make_texture(h, w, seed, sigma=1.8):
    """Band-limited noise + soft-edged random rectangles (plenty of Shi-Tomasi corners), float32 in [8, 247]."""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((h, w)).astype(np.float32)
    t = _blur(t, sigma)
    t /= max(1e-6, float(t.std()))
    blocks = np.zeros((h, w), np.float32)
    nrect = max(8, (h * w) // 6000)
    ys = rng.integers(0, h, nrect); xs = rng.integers(0, w, nrect)
    hs = rng.integers(6, 40, nrect); ws = rng.integers(6, 40, nrect)
    amp = rng.uniform(-2.0, 2.0, nrect).astype(np.float32)
    for y, x, hh, ww_, a in zip(ys, xs, hs, ws, amp):
        blocks[y:y + hh, x:x + ww_] += a
    blocks = _blur(blocks, 1.0)
    t = 0.7 * t + 0.6 * blocks
    t = 127.5 + 45.0 * t
    return np.clip(t, 8, 247).astype(np.float32)


def rotation_matrix(omega):
    """exp([omega]x) by Rodrigues' formula (the series' first terms below 1e-8 rad)."""
    om = np.asarray(omega, np.float64)
    W = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    th2 = float(om @ om)
    A, B = (1.0, 0.5) if th2 < 1e-16 else (np.sin(np.sqrt(th2)) / np.sqrt(th2), (1.0 - np.cos(np.sqrt(th2))) / th2)
    return np.eye(3) + A * W + B * (W @ W)


def pixel_homography(v, omega, d, n, scaling, cx, cy, motion="linear"):
    """motion "linear" (the default): K (I + [w]x + v n' / d) K^-1, the first-order form of the module's text.  "finite": the frame
    pair as the rigid motion P1 = R P0 + T it is, K (I + T n' / (d - n.T)) exp([w]x) K^-1, with v read as the displacement T per
    frame interval and n, d the plane in the NEXT frame's camera axes, as the sensor record carries them (ofk.h:
    ofk_set_finite_motion)."""
    v = np.asarray(v, np.float64); om = np.asarray(omega, np.float64); n = np.asarray(n, np.float64)
    if motion not in ("linear", "finite"):
        raise ValueError(f"motion {motion!r} is neither 'linear' nor 'finite'")
    W = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    if motion == "finite":
        Hn = (np.eye(3) + np.outer(v, n) / (d - float(n @ v))) @ rotation_matrix(om)
    else:
        Hn = np.eye(3) + W + np.outer(v, n) / d
    K = np.array([[1 / scaling, 0, cx], [0, 1 / scaling, cy], [0, 0, 1.0]])
    return K @ Hn @ np.linalg.inv(K)


def _bilinear(img, xs, ys):
    h, w = img.shape
    xs = np.clip(xs, 0, w - 1.001); ys = np.clip(ys, 0, h - 1.001)
    x0 = np.floor(xs).astype(np.int32); y0 = np.floor(ys).astype(np.int32)
    a = (xs - x0).astype(np.float32); b = (ys - y0).astype(np.float32)
    i00 = img[y0, x0]; i01 = img[y0, x0 + 1]; i10 = img[y0 + 1, x0]; i11 = img[y0 + 1, x0 + 1]
    return (i00 * (1 - a) + i01 * a) * (1 - b) + (i10 * (1 - a) + i11 * a) * b


def ideal_grid(h, w, camera):
    """The ideal pixel (float64 xx, yy) every raw pixel of an h x w frame looks at through `camera` (a pipeline.CameraModel): the
    lens undone as ofk.h writes it (ofk_set_camera), in float64 and with the model's iteration count."""
    m = camera.setting()
    k = list(m.k)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    x0 = (xx - m.cx) / m.fx; y0 = (yy - m.cy) / m.fy
    if m.model == 1:                                             # Brown: the fixed-point iteration
        k1, k2, p1, p2, k3, k4, k5, k6 = k
        x, y = x0, y0
        for _ in range(m.iters):
            r2 = x * x + y * y
            icd = (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x); dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            x = (x0 - dx) * icd; y = (y0 - dy) * icd
    else:                                                        # equidistant fisheye: Newton on theta
        k1, k2, k3, k4 = k[:4]
        td = np.sqrt(x0 * x0 + y0 * y0); t = td
        for _ in range(m.iters):
            t2 = t * t; t4 = t2 * t2; t6 = t4 * t2; t8 = t4 * t4
            t = t - (t * (1.0 + k1 * t2 + k2 * t4 + k3 * t6 + k4 * t8) - td) / (1.0 + 3.0 * k1 * t2 + 5.0 * k2 * t4 + 7.0 * k3 * t6 + 9.0 * k4 * t8)
        sc = np.where(td < 1e-8, 1.0, np.tan(t) / np.maximum(td, 1e-300))
        x = x0 * sc; y = y0 * sc
    return x * m.fo_x + m.co_x, y * m.fo_y + m.co_y


def _camera_view(h, w, camera, margin):
    """(scaling, cx, cy of the ideal pinhole, the ideal grid, a margin that holds it): the frame is what `camera` sees."""
    scaling, cx, cy = camera.sensor_slots()
    xx, yy = ideal_grid(h, w, camera)
    over = max(0.0, -xx.min(), -yy.min(), xx.max() - (w - 1), yy.max() - (h - 1))
    return scaling, cx, cy, xx, yy, max(int(margin), int(np.ceil(over)) + 16)


def _row_times(h, rolling_shutter):
    """The capture time of every raw row against its frame's time stamp, in frame intervals: readout * (y / rows - anchor)."""
    m = rolling_shutter.setting()
    return m.readout * (np.arange(h, dtype=np.float64) / (m.rows or h) - m.anchor)


def _row_sources(xx, yy, M, margin):
    """Texture coordinates of the ideal pixels (xx, yy) [h,w] where row y was exposed under its own homography M[y] (texture -> image)."""
    Hi = np.linalg.inv(M)[:, None]                               # [h,1,3,3]
    den = Hi[..., 2, 0] * xx + Hi[..., 2, 1] * yy + Hi[..., 2, 2]
    return (Hi[..., 0, 0] * xx + Hi[..., 0, 1] * yy + Hi[..., 0, 2]) / den + margin, (Hi[..., 1, 0] * xx + Hi[..., 1, 1] * yy + Hi[..., 1, 2]) / den + margin


def _colour(T, T2, ax, ay):
    base, tint = _bilinear(T, ax, ay), _bilinear(T2, ax, ay)
    return np.stack([np.clip(np.rint(base + g * (tint - 127.5)), 0, 255).astype(np.uint8) for g in (0.10, -0.06, 0.08)], -1)


def render_pair(h, w, seed, v=(0.003, -0.002, 0.001), omega=(0.002, -0.001, 0.003), d=1.0, n=(0, 0, 1), scaling=None,
                margin=48, camera=None, rolling_shutter=None, motion="linear", relief=None):
    """Returns dict(prev, next: [h,w,3] uint8 BGR; H: 3x3 pixel homography prev->next; scaling, cx, cy).
    relief (default None: the one plane): dict(rect=(x0, y0, x1, y1), height=h) composites a second plane at distance d (1 - h) with
    the same normal over the pixels x0 <= x < x1, y0 <= y < y1 of the `next` frame: there the texture is seen through that plane's
    own homography (info["H_relief"]), as a roof painted like the ground would be; `prev` is the one plane's.  Not with a camera or
    a rolling shutter.
    motion: pixel_homography's ("finite": the exact rigid motion of the pair; not with a rolling shutter, whose rows are rendered
    through the linearised homography).
    camera (a pipeline.CameraModel, default None): the frames are what that camera sees - every raw pixel is undistorted to the ideal
    pixel it looks at, sent through the homography and sampled bilinearly (the previous frame too, at the ideal pixel itself);
    scaling, cx, cy are then the ideal pinhole's (camera.sensor_slots()) and H lives in ideal pixels.
    rolling_shutter (a pipeline.RollingShutter, default None): raw row y of frame k (0 = prev, 1 = next) is exposed at the time
    t = k + readout * (y / h - anchor) and rendered through the pair's linearised homography at that time,
    K (I + t (W + v n' / d)) K^-1 - pixel_homography's own form with t v, t omega; H stays the global shutter's.  Works behind a
    camera as well (the rows are the raw image's)."""
    if relief is not None and (camera is not None or rolling_shutter is not None):
        raise ValueError("render_pair: relief is rendered for the ideal pinhole with a global shutter alone")
    if rolling_shutter is not None and motion != "linear":
        raise ValueError("render_pair: a rolling shutter is rendered through the linearised homography: motion must be 'linear'")
    if rolling_shutter is not None:
        if camera is not None:
            scaling, cx, cy, xx, yy, margin = _camera_view(h, w, camera, margin)
        else:
            scaling = scaling or 1.0 / max(h, w)
            cx, cy = w / 2.0, h / 2.0
            yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        T = make_texture(h + 2 * margin, w + 2 * margin, seed)
        T2 = make_texture(h + 2 * margin, w + 2 * margin, seed + 7919, sigma=3.0)
        H = pixel_homography(v, omega, d, n, scaling, cx, cy)
        G = H - np.eye(3)                                        # K (W + v n' / d) K^-1
        tau = _row_times(h, rolling_shutter)
        out = {name: _colour(T, T2, *_row_sources(xx, yy, np.eye(3) + (k + tau)[:, None, None] * G, margin)) for k, name in enumerate(("prev", "next"))}
        info = dict(prev=out["prev"], next=out["next"], H=H, scaling=scaling, cx=cx, cy=cy, v=np.asarray(v, np.float64),
                    omega=np.asarray(omega, np.float64), d=float(d), n=np.asarray(n, np.float64), rolling_shutter=rolling_shutter)
        if camera is not None:
            info["camera"] = camera
        return info
    if camera is not None:
        scaling, cx, cy, xx, yy, margin = _camera_view(h, w, camera, margin)
        T = make_texture(h + 2 * margin, w + 2 * margin, seed)
        T2 = make_texture(h + 2 * margin, w + 2 * margin, seed + 7919, sigma=3.0)
        H = pixel_homography(v, omega, d, n, scaling, cx, cy, motion)
        Hi = np.linalg.inv(H)
        den = Hi[2, 0] * xx + Hi[2, 1] * yy + Hi[2, 2]
        sx = (Hi[0, 0] * xx + Hi[0, 1] * yy + Hi[0, 2]) / den + margin
        sy = (Hi[1, 0] * xx + Hi[1, 1] * yy + Hi[1, 2]) / den + margin
        out = {}
        for name, (ax, ay) in (("prev", (xx + margin, yy + margin)), ("next", (sx, sy))):
            base, tint = _bilinear(T, ax, ay), _bilinear(T2, ax, ay)
            out[name] = np.stack([np.clip(np.rint(base + g * (tint - 127.5)), 0, 255).astype(np.uint8) for g in (0.10, -0.06, 0.08)], -1)
        return dict(prev=out["prev"], next=out["next"], H=H, scaling=scaling, cx=cx, cy=cy, v=np.asarray(v, np.float64),
                    omega=np.asarray(omega, np.float64), d=float(d), n=np.asarray(n, np.float64), camera=camera)
    scaling = scaling or 1.0 / max(h, w)
    cx, cy = w / 2.0, h / 2.0
    T = make_texture(h + 2 * margin, w + 2 * margin, seed)
    T2 = make_texture(h + 2 * margin, w + 2 * margin, seed + 7919, sigma=3.0)
    H = pixel_homography(v, omega, d, n, scaling, cx, cy, motion)
    Hi = np.linalg.inv(H)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    den = Hi[2, 0] * xx + Hi[2, 1] * yy + Hi[2, 2]
    sx = (Hi[0, 0] * xx + Hi[0, 1] * yy + Hi[0, 2]) / den + margin
    sy = (Hi[1, 0] * xx + Hi[1, 1] * yy + Hi[1, 2]) / den + margin

    def colour(base, tint):
        out = np.empty(base.shape + (3,), np.uint8)
        for ch, g in enumerate((0.10, -0.06, 0.08)):
            out[..., ch] = np.clip(np.rint(base + g * (tint - 127.5)), 0, 255).astype(np.uint8)
        return out

    prev = colour(T[margin:margin + h, margin:margin + w], T2[margin:margin + h, margin:margin + w])
    nxt = colour(_bilinear(T, sx, sy), _bilinear(T2, sx, sy))
    if relief is not None:
        x0, y0, x1, y1 = (int(c) for c in relief["rect"])
        hr = float(relief["height"])
        if not (0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h and hr < 1.0):
            raise ValueError(f"render_pair: relief rect {relief['rect']} outside the {w} x {h} frame or height {hr} not below 1")
        Hr = pixel_homography(v, omega, d * (1.0 - hr), n, scaling, cx, cy, motion)
        Hri = np.linalg.inv(Hr)
        ry, rx = yy[y0:y1, x0:x1], xx[y0:y1, x0:x1]
        den = Hri[2, 0] * rx + Hri[2, 1] * ry + Hri[2, 2]
        qx = (Hri[0, 0] * rx + Hri[0, 1] * ry + Hri[0, 2]) / den + margin
        qy = (Hri[1, 0] * rx + Hri[1, 1] * ry + Hri[1, 2]) / den + margin
        nxt[y0:y1, x0:x1] = colour(_bilinear(T, qx, qy), _bilinear(T2, qx, qy))
        return dict(prev=prev, next=nxt, H=H, H_relief=Hr, relief=dict(rect=(x0, y0, x1, y1), height=hr), scaling=scaling, cx=cx, cy=cy,
                    v=np.asarray(v, np.float64), omega=np.asarray(omega, np.float64), d=float(d), n=np.asarray(n, np.float64))
    return dict(prev=prev, next=nxt, H=H, scaling=scaling, cx=cx, cy=cy, v=np.asarray(v, np.float64),
                omega=np.asarray(omega, np.float64), d=float(d), n=np.asarray(n, np.float64))


def warp_frame(bgr, H):
    """A BGR uint8 frame seen through the pixel homography H (prev -> next), bilinear, edge pixels replicated: the `next` frame of a
    pair whose `prev` is a given picture (a real camera frame instead of make_texture)."""
    h, w = bgr.shape[:2]
    Hi = np.linalg.inv(H)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    den = Hi[2, 0] * xx + Hi[2, 1] * yy + Hi[2, 2]
    sx = (Hi[0, 0] * xx + Hi[0, 1] * yy + Hi[0, 2]) / den
    sy = (Hi[1, 0] * xx + Hi[1, 1] * yy + Hi[1, 2]) / den
    out = np.empty_like(bgr)
    for ch in range(bgr.shape[2]):
        out[..., ch] = np.clip(np.rint(_bilinear(bgr[..., ch].astype(np.float32), sx, sy)), 0, 255).astype(np.uint8)
    return out


def apply_exposure(img, gain=1.0, bias=0.0, vignette=0.0):
    """A gray [h,w] or BGR [h,w,3] uint8 frame under another exposure: clip(rint(img * gain * f + bias), 0, 255) with the vignette
    f = 1 - vignette * r^2, r^2 = ((x - w/2)^2 + (y - h/2)^2) / ((w/2)^2 + (h/2)^2) - what auto-exposure and a lens's fall-off do
    between the two frames of a pair (ofk.h: ofk_lk_light)."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise ValueError(f"apply_exposure: {img.dtype} {img.shape} is no gray or BGR uint8 frame")
    h, w = img.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    r2 = ((xx - w / 2.0) ** 2 + (yy - h / 2.0) ** 2) / ((w / 2.0) ** 2 + (h / 2.0) ** 2)
    f = 1.0 - float(vignette) * r2
    if img.ndim == 3:
        f = f[..., None]
    return np.clip(np.rint(img.astype(np.float64) * float(gain) * f + float(bias)), 0, 255).astype(np.uint8)


def render_sequence(h, w, seed, n_frames, v=(0.003, -0.002, 0.001), omega=(0.002, -0.001, 0.003), d=1.0, n=(0, 0, 1),
                    scaling=None, margin=96, camera=None, rolling_shutter=None, motion="linear", relief=None):
    """`n_frames` BGR frames of one stream under constant per-frame motion: frame k shows the texture through H^k.
    relief (default None: the one plane): render_pair's dict(rect=(x0, y0, x1, y1), height=h), the rect in the pixels of frame 0: a
    second plane at distance d (1 - h) with the same normal, painted like the ground; frame k shows it through its own homography
    Hr^k (info["H_relief"]) over the pixels that Hr^-k takes into the rect.  Not with a camera or a rolling shutter.
    motion: pixel_homography's ("finite": every step is the exact rigid motion with the plane n, d in the axes of the step's later
    frame; not with a rolling shutter).
    Returns (frames [n,h,w,3] uint8, info dict as render_pair).  camera: as in render_pair.  rolling_shutter: as in render_pair, with
    row y of frame k seen through (I + tau G) H^k, tau = readout * (y / h - anchor), G = H - I: the linearised motion over the row
    time behind the k whole steps (I + (k + tau) G itself would drift from H^k with k)."""
    if relief is not None and (camera is not None or rolling_shutter is not None):
        raise ValueError("render_sequence: relief is rendered for the ideal pinhole with a global shutter alone")
    if camera is not None:
        scaling, cx, cy, xx, yy, margin = _camera_view(h, w, camera, margin)
    else:
        scaling = scaling or 1.0 / max(h, w)
        cx, cy = w / 2.0, h / 2.0
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    T = make_texture(h + 2 * margin, w + 2 * margin, seed)
    T2 = make_texture(h + 2 * margin, w + 2 * margin, seed + 7919, sigma=3.0)
    if rolling_shutter is not None and motion != "linear":
        raise ValueError("render_sequence: a rolling shutter is rendered through the linearised homography: motion must be 'linear'")
    H = pixel_homography(v, omega, d, n, scaling, cx, cy, motion)
    if relief is not None:
        x0, y0, x1, y1 = (int(c) for c in relief["rect"])
        hr = float(relief["height"])
        if not (0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h and hr < 1.0):
            raise ValueError(f"render_sequence: relief rect {relief['rect']} outside the {w} x {h} frame or height {hr} not below 1")
        Hr, Hrk = pixel_homography(v, omega, d * (1.0 - hr), n, scaling, cx, cy, motion), np.eye(3)
    frames = np.empty((n_frames, h, w, 3), np.uint8)
    Hk = np.eye(3)
    tau = None if rolling_shutter is None else _row_times(h, rolling_shutter)
    for k in range(n_frames):
        if tau is not None:
            sx, sy = _row_sources(xx, yy, (np.eye(3) + tau[:, None, None] * (H - np.eye(3))) @ Hk, margin)
        else:
            Hi = np.linalg.inv(Hk)
            den = Hi[2, 0] * xx + Hi[2, 1] * yy + Hi[2, 2]
            sx = (Hi[0, 0] * xx + Hi[0, 1] * yy + Hi[0, 2]) / den + margin
            sy = (Hi[1, 0] * xx + Hi[1, 1] * yy + Hi[1, 2]) / den + margin
        base, tint = _bilinear(T, sx, sy), _bilinear(T2, sx, sy)
        for ch, g in enumerate((0.10, -0.06, 0.08)):
            frames[k, ..., ch] = np.clip(np.rint(base + g * (tint - 127.5)), 0, 255).astype(np.uint8)
        if relief is not None:
            Hri = np.linalg.inv(Hrk)
            den = Hri[2, 0] * xx + Hri[2, 1] * yy + Hri[2, 2]
            qx = (Hri[0, 0] * xx + Hri[0, 1] * yy + Hri[0, 2]) / den
            qy = (Hri[1, 0] * xx + Hri[1, 1] * yy + Hri[1, 2]) / den
            roof = (qx >= x0) & (qx < x1) & (qy >= y0) & (qy < y1)
            base, tint = _bilinear(T, qx[roof] + margin, qy[roof] + margin), _bilinear(T2, qx[roof] + margin, qy[roof] + margin)
            for ch, g in enumerate((0.10, -0.06, 0.08)):
                frames[k, ..., ch][roof] = np.clip(np.rint(base + g * (tint - 127.5)), 0, 255).astype(np.uint8)
            Hrk = Hr @ Hrk
        Hk = H @ Hk
    if relief is not None:
        return frames, dict(H=H, H_relief=Hr, relief=dict(rect=(x0, y0, x1, y1), height=hr), scaling=scaling, cx=cx, cy=cy, v=np.asarray(v, np.float64),
                            omega=np.asarray(omega, np.float64), d=float(d), n=np.asarray(n, np.float64))
    return frames, dict(H=H, scaling=scaling, cx=cx, cy=cy, v=np.asarray(v, np.float64), omega=np.asarray(omega, np.float64),
                        d=float(d), n=np.asarray(n, np.float64))


def true_flow_px(H, pts_xy):
    """Exact displacement (pixels) of prev-frame points under the pair's homography."""
    p = np.concatenate([np.asarray(pts_xy, np.float64).reshape(-1, 2), np.ones((len(pts_xy), 1))], 1) @ H.T
    return p[:, :2] / p[:, 2:3] - np.asarray(pts_xy, np.float64).reshape(-1, 2)


def make_batch(batch, h, w, seed, distinct=4, **kw):
    """`batch` frame pairs: `distinct` rendered pairs, the rest cyclic shifts of them (different pixels,
    same statistics) so that large benchmark batches build in seconds."""
    base = [render_pair(h, w, seed + i, **kw) for i in range(min(distinct, batch))]
    prev = np.empty((batch, h, w, 3), np.uint8); nxt = np.empty((batch, h, w, 3), np.uint8)
    for b in range(batch):
        src = base[b % len(base)]
        k = b // len(base)
        if k == 0:
            prev[b] = src["prev"]; nxt[b] = src["next"]
        else:
            sh = (17 * k) % h, (29 * k) % w
            prev[b] = np.roll(src["prev"], sh, axis=(0, 1)); nxt[b] = np.roll(src["next"], sh, axis=(0, 1))
    return prev, nxt, base
