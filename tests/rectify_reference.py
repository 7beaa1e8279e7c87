"""tests/rectify_reference.py — numpy restatement of the warp through a lens (ofk.h: ofk_warp_lens).

warp_lens()     the rule of ofk.h step by step: the normalised matrix, the coordinates elementwise in float64 (numpy's products and sums
                round one by one, as the kernel's do without contraction), camera_reference.distort_normalised for the lens, the camera
                matrix, the scale by 32, then the plain warp's tail (rint to even, 5 fractional bits, four taps).  Frames and covered
                counts are the device's bit for bit wherever every operation is IEEE-exact (Brown: + - * / only); the fisheye's atan
                comes from another math library, so they are the device's where no coordinate lies near a rounding tie - `tie` says how near.
cameras()       the cameras of the GPU test; gpu_cases() its fisheye inputs, for the tie-free condition asserted on the CPU.
ideal_radius()  the brute-force largest ideal radius over the raw frame's border.
lens_sequence() stabilise_reference.sequence() seen through a lens.
warp_lens() and cameras() import nothing from the package."""
import numpy as np

import camera_reference as cr
import stabilise_reference as sr

BORDER_CONSTANT, BORDER_REPLICATE = sr.BORDER_CONSTANT, sr.BORDER_REPLICATE
LIMIT = sr.LIMIT


def coordinates(M, cam, dh, dw, r_max=0.0):
    """Steps 1-5 of ofk.h: (fx, fy in 1/32 raw pixels, ok) per destination pixel, [dh,dw] each.  M None: the identity."""
    m = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0] if M is None else [float(v) for v in np.asarray(M, np.float64).reshape(9)]
    x = np.arange(dw, dtype=np.float64)[None, :]
    y = np.arange(dh, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        f = [np.float64(v) for v in m]
        co_x, co_y, fo_x, fo_y = (np.float64(cam[k]) for k in ("co_x", "co_y", "fo_x", "fo_y"))
        mn = [(f[0] - co_x * f[6]) / fo_x, (f[1] - co_x * f[7]) / fo_x, (f[2] - co_x * f[8]) / fo_x,
              (f[3] - co_y * f[6]) / fo_y, (f[4] - co_y * f[7]) / fo_y, (f[5] - co_y * f[8]) / fo_y, f[6], f[7], f[8]]
        X = (mn[0] * x + mn[1] * y) + mn[2]
        Y = (mn[3] * x + mn[4] * y) + mn[5]
        W = (mn[6] * x + mn[7] * y) + mn[8]
        iw = np.where(W != 0.0, 1.0 / W, 0.0)
        xn, yn = X * iw, Y * iw
        xd, yd = cr.distort_normalised(cam, xn, yn)
        fx = (xd * cam["fx"] + cam["cx"]) * 32.0
        fy = (yd * cam["fy"] + cam["cy"]) * 32.0
        ok = (np.abs(fx) <= LIMIT) & (np.abs(fy) <= LIMIT)      # False for NaN
        if r_max > 0.0:
            ok &= (xn * xn + yn * yn) <= np.float64(r_max) * np.float64(r_max)
    return fx, fy, ok


def tail(src, fx, fy, ok, border=BORDER_CONSTANT, border_value=0):
    """Steps 4-7 of ofk_warp_perspective on given coordinates (stabilise_reference.warp_mask's tail, which takes a matrix only)."""
    src = np.asarray(src, np.uint8)
    img = src[:, :, None] if src.ndim == 2 else src
    sh, sw, ch = img.shape
    dh, dw = fx.shape
    ix = np.rint(np.where(ok, fx, 0.0)).astype(np.int64)
    iy = np.rint(np.where(ok, fy, 0.0)).astype(np.int64)
    sx, ax, sy, ay = ix >> 5, ix & 31, iy >> 5, iy & 31
    acc = np.zeros((dh, dw, ch), np.int64)
    inside_all = np.ones((dh, dw), bool)
    for dy, dx, wgt in ((0, 0, (32 - ax) * (32 - ay)), (0, 1, ax * (32 - ay)), (1, 0, (32 - ax) * ay), (1, 1, ax * ay)):
        tx, ty = sx + dx, sy + dy
        inside = (tx >= 0) & (tx < sw) & (ty >= 0) & (ty < sh)
        p = img[np.clip(ty, 0, sh - 1), np.clip(tx, 0, sw - 1)].astype(np.int64)
        if border == BORDER_CONSTANT:
            p = np.where(inside[:, :, None], p, int(border_value))
        acc += wgt[:, :, None] * p
        inside_all &= inside
    out = np.where(ok[:, :, None], (acc + 512) >> 10, int(border_value)).astype(np.uint8)
    return (out[:, :, 0] if src.ndim == 2 else out), ok & inside_all


def warp_lens(src, M, cam, dsize=None, border=BORDER_CONSTANT, border_value=0, r_max=0.0):
    """src [h,w] or [h,w,C] uint8, the raw image of `cam` (camera_reference.camera's dict); M 3x3 destination -> ideal pixel (None: the
    identity); dsize (height, width).  -> (dst in src's layout, covered [dh,dw] bool, tie [dh,dw]: the distance of fx or fy, whichever
    is nearer, to a rounding tie (k + 1/2), in fixed-point units; inf where the pixel is outside)."""
    src = np.asarray(src, np.uint8)
    dh, dw = src.shape[:2] if dsize is None else dsize
    fx, fy, ok = coordinates(M, cam, dh, dw, r_max)
    out, mask = tail(src, fx, fy, ok, border, border_value)
    with np.errstate(all="ignore"):
        t = np.minimum(np.abs(np.abs(fx - np.floor(fx)) - 0.5), np.abs(np.abs(fy - np.floor(fy)) - 0.5))
    return out, mask, np.where(ok, t, np.inf)


def warp_lens_batch(src, M, cam, dsize=None, border=BORDER_CONSTANT, border_value=0, r_max=0.0):
    """warp_lens() per image of src [B,...] with M [B,3,3] or None -> (dst [B,...], covered [B] int32, the smallest tie distance)."""
    res = [warp_lens(s, None if M is None else M[b], cam, dsize, border, border_value, r_max) for b, s in enumerate(src)]
    return np.stack([r[0] for r in res]), np.array([np.count_nonzero(r[1]) for r in res], np.int32), min(float(r[2].min()) for r in res)


def ideal_radius(cam, h, w):
    """The largest ideal normalised radius over the border pixels of the raw h x w frame, pixel by pixel."""
    best = 0.0
    for yy in range(h):
        for xx in (range(w) if yy in (0, h - 1) else (0, w - 1)):
            x, y = cr.undistort_normalised(cam, (xx - cam["cx"]) / cam["fx"], (yy - cam["cy"]) / cam["fy"])
            best = max(best, float(np.sqrt(x * x + y * y)))
    return best


# ------------------------------------------------------------------------------------------------ the 240 x 320 camera of the sequences
SEQ = dict(h=240, w=320, fx=250.0, fy=252.0, cx=163.1, cy=117.5)
LENSES = dict(MILD=cr.MILD, STRONG=cr.STRONG, FISH=cr.FISH)
_cache = {}


def seq_camera(lens, **kw):
    """The sequences' camera with one of camera_reference's lenses: (the reference's dict, the keywords of pipeline.CameraModel)."""
    model, k, _ = lens
    c = dict(fx=SEQ["fx"], fy=SEQ["fy"], cx=SEQ["cx"], cy=SEQ["cy"])
    return cr.camera(model, k, **c, **kw), dict(model="brown" if model == cr.BROWN else "fisheye", k=tuple(k), **c)


def gray_of(frames):
    f = np.asarray(frames).astype(np.uint32)
    return ((f[..., 0] * 3735 + f[..., 1] * 19235 + f[..., 2] * 9798 + 16384) >> 15).astype(np.uint8)


def lens_sequence(which, lens_name, n_frames=12, seed=5):
    """(raw gray [n,h,w] seen through the lens, the same scene's gray without a lens, H [n,3,3] in ideal pixels, the camera's dict, the
    BGR frames through the lens, info): stabilise_reference.sequence()'s motion `which` rendered through the sequences' camera.  Computed
    once per argument set; callers leave the arrays as they are."""
    key = (which, lens_name, n_frames, seed)
    if key not in _cache:
        from of_amd import synth
        from of_amd.pipeline import CameraModel
        cam, kw = seq_camera(LENSES[lens_name])
        cm = CameraModel(**kw)
        v, om = sr.SEQUENCES[which]
        frames, info = synth.render_sequence(SEQ["h"], SEQ["w"], seed, n_frames, v=v, omega=om, motion="finite", camera=cm)
        plain, _ = synth.render_sequence(SEQ["h"], SEQ["w"], seed, n_frames, v=v, omega=om, motion="finite", scaling=info["scaling"])
        H1 = synth.pixel_homography(v, om, 1.0, (0, 0, 1), info["scaling"], info["cx"], info["cy"], motion="finite")
        H = np.stack([np.linalg.matrix_power(H1, k) for k in range(n_frames)])
        out = (gray_of(frames), gray_of(plain), H, cam, frames, info)
        for a in out[:3]:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def chain(which, lens_name, n_frames=12, corners=150, s=None, key=None):
    """stabilise_reference.chain() behind a lens: the same stages on the RAW frames (the C oracle's LK, the template restatement), the
    keyframe restatement on the IDEAL pixels of the tracks (camera_reference.undistort_points, as ofk_set_camera hands them to it),
    pose() on its record, warp_lens() of every raw frame into the view.  The first step finds no keyframe and leaves frame 1 rectified:
    the figures are taken against that from frame 2 on.  -> stabilise_reference.chain()'s dict."""
    import keyframe_reference as K
    import track_template_reference as tr
    from oracle import image_oracle as io
    s = sr.setting() if s is None else s
    ks = K.setting() if key is None else key
    _, _, _, cam, frames, info = lens_sequence(which, lens_name, n_frames)
    h, w = SEQ["h"], SEQ["w"]
    gray = [io.gray_bgr8(f) for f in frames]
    pts = io.good_features(gray[0], corners, 0.01, 10, 3).reshape(-1, 2).astype(np.float32)
    S = len(pts)
    cfg = tr.setting()
    age, tstate = np.zeros(S, np.int32), tr.empty_state(S, cfg.win)
    kst, one = K.empty(S), K.empty(S)
    dr_s = K.setting(gate=ks["gate"], min_rows=ks["min_rows"], max_age=1, min_share=0.0, rot_max=3.0)
    sn = np.zeros(28)
    sn[0] = info["d"]; sn[1:4] = info["n"]; sn[4:7] = info["omega"]; sn[7] = sn[11] = sn[15] = 1.0
    sn[19] = info["scaling"]; sn[20] = info["cx"]; sn[21] = info["cy"]
    ideal = lambda p: cr.undistort_points(cam, p).astype(np.float32).reshape(-1, 2)
    state, cov, ref, out = None, 0, None, dict(rows=[], flags=[], rebases=0)
    for k in range(n_frames - 1):
        n = len(pts)
        g0, g1 = gray[k], gray[k + 1]
        nxt, stt = tr.cpu_lk(g0, g1, pts)
        nxt, stt = nxt.astype(np.float32), (stt != 0).astype(np.uint8)
        pad = lambda a, *tail: np.concatenate([a, np.zeros((S - n,) + tail, a.dtype)])
        rec, L = tr.affine_fit(pts, nxt, stt, n, h, w, cfg)
        nxt_s, st_s, tstate, _ = tr.template_step(g0, g1, pad(pts, 2), pad(nxt, 2), pad(stt), age, n, L, tstate, cfg)
        nxt, stt = nxt_s[:n], st_s[:n]
        age = np.concatenate([age[:n][stt != 0] + 1, np.zeros(S - int((stt != 0).sum()), np.int32)])
        one["key_xy"] = pad(ideal(pts), 2); one["member"][:] = 1
        one["state"] = K.empty(1)["state"]; one["istate"] = np.array([k, n, 0, 0], np.int32)
        _, r1, _, _ = K.step(one, pad(ideal(nxt), 2), pad(stt), n, sn, np.zeros(3), False, k, dr_s)
        R_used = K.mul3(K.rotation(sn[4:7]), kst["state"][:9].reshape(3, 3))
        kst, krec, cnt, _ = K.step(kst, pad(ideal(nxt), 2), pad(stt), n, sn, r1[10:13], r1[3] == K.SOLVED, k, ks)
        state, prec = sr.pose(R_used, krec, sn, h, w, state, prev_covered=cov, s=s)
        frame, mask, _ = warp_lens(gray[k + 1], prec[0:9].reshape(3, 3), cam, None, s["border"], s["border_value"])
        cov = int(np.count_nonzero(mask))
        if k == 0:
            ref = frame.astype(np.int32)
        else:
            stab = float(np.abs(frame.astype(np.int32) - ref)[mask].mean()) if cov else float("nan")
            raw = float(np.abs(gray[k + 1].astype(np.int32) - gray[1].astype(np.int32)).mean())
            out["rows"].append((stab, raw, cov / float(h * w)))
        out["flags"].append(int(prec[30]))
        pts = nxt[stt != 0]
    out["rebases"], out["approx"], out["keyframes"] = int(prec[33]), int(prec[34]), int(kst["istate"][2])
    out["gain"] = min(r / st for st, r, _ in out["rows"])
    return out


# ------------------------------------------------------------------------------------------------ the GPU test's cameras and inputs
def cameras(sh, sw):
    """name -> (camera dict, r_max) over an sh x sw source: Brown with tangential and rational terms, Brown with k4..k6 = 0 (the
    skipped divide), the fisheye, a coefficient set whose denominator crosses zero inside the frame (cd = inf / NaN), r_max binding
    inside the frame; fo_x != fo_y throughout."""
    f = 0.9 * max(sh, sw, 4)
    c = dict(fx=f, fy=1.03 * f, cx=0.52 * (sw - 1), cy=0.47 * (sh - 1), fo_x=0.8 * f, fo_y=0.83 * f, co_x=0.5 * (sw - 1) + 0.25, co_y=0.5 * (sh - 1) - 0.5)
    return {
        "rational": (cr.camera(cr.BROWN, (-0.28, 0.09, 0.0008, -0.0005, -0.012, 0.05, -0.01, 0.002), **c), 0.0),
        "poly": (cr.camera(cr.BROWN, (-0.28, 0.09, 0.0008, -0.0005, -0.012), **c), 0.0),
        "fisheye": (cr.camera(cr.FISHEYE, (-0.03, 0.005, -0.001, 0.0002), **c), 0.0),
        "pole": (cr.camera(cr.BROWN, (0.1, 0.0, 0.001, 0.0, 0.0, -8.0, 0.0, 0.0), **c), 0.0),       # 1 - 8 r2 = 0 at r = 0.354
        "r_max": (cr.camera(cr.BROWN, (-0.28, 0.09, 0.0008, -0.0005, -0.012), **c), 0.3),
    }


SIZES = ((1, 1), (3, 5), (5, 257), (9, 254), (13, 256), (17, 258), (240, 320))      # (h, w): 4 k + 1 rows, the second block column, byte stores
PAIRS = [(s, SIZES[(i + 1) % len(SIZES)]) for i, s in enumerate(SIZES)] + [(SIZES[-1], SIZES[-1])]
FISH_TIE = 1e-8                                                 # fixed-point units: the fisheye inputs keep this far from every tie


def matrices(sh, sw, dh, dw):
    """stabilise_reference.matrices() taken as destination -> IDEAL pixel, plus None (the identity: plain rectification)."""
    return dict(sr.matrices(sh, sw, dh, dw), none=None)
