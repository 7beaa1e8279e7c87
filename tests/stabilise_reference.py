"""tests/stabilise_reference.py — numpy restatement of the perspective warp (ofk.h: ofk_warp_perspective; DESIGN.md "Perspective warp").

warp()        the rule of ofk.h step by step: the coordinates elementwise in float64 (numpy's products and sums round one by one, as
              the kernel's do without contraction), one divide, rint to even, 5 fractional bits, the integer sum of the four taps.
              Frames and covered counts are the device's bit for bit.
matrices()    the matrices the GPU test sends through the kernel: identity, shifts (whole, 1/2 px, 1/64 px = every fx a rounding
              tie), a rotation, a perspective whose W changes sign inside the frame, scales, |fx| on either side of 2^30, NaN, inf, zero.
sequence()    the rendered finite-motion sequence of the issue's table and the true homography of every frame into frame 0's view.
pose()        rules 1-4 of the stabilised view (ofk.h: ofk_set_stabilise) for one stream in the kernel's order of operations: flags,
              reasons and counts are the device's bit for bit, M, Bv, R, T close (the rotation comes from another math library).
view_run()    the view's bookkeeping over a sequence whose homographies are known (the re-base by cover).
chain()       the CPU chain: the C oracle's LK, the template and keyframe restatements, pose() and warp() over a rendered sequence.
warp(), matrices() and pose() import nothing from the package; sequence() and chain() import its synth and the oracle for their frames
and tracks, as keyframe_reference.rendered() does."""
import numpy as np

BORDER_CONSTANT, BORDER_REPLICATE = 0, 1
LIMIT = 1073741824.0                                            # 2^30


def warp(src, M, dsize=None, border=BORDER_CONSTANT, border_value=0):
    """src [h,w] or [h,w,C] uint8, M 3x3 destination -> source, dsize (height, width) -> (dst uint8 in src's layout, covered count)."""
    out, mask = warp_mask(src, M, dsize, border, border_value)
    return out, int(np.count_nonzero(mask))


def warp_mask(src, M, dsize=None, border=BORDER_CONSTANT, border_value=0):
    """warp() with the covered pixels themselves, [dh,dw] bool, in place of their count."""
    src = np.asarray(src, np.uint8)
    img = src[:, :, None] if src.ndim == 2 else src
    sh, sw, ch = img.shape
    dh, dw = (sh, sw) if dsize is None else dsize
    m = [float(v) for v in np.asarray(M, np.float64).reshape(9)]
    x = np.arange(dw, dtype=np.float64)[None, :]
    y = np.arange(dh, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        X = (m[0] * x + m[1] * y) + m[2]
        Y = (m[3] * x + m[4] * y) + m[5]
        W = (m[6] * x + m[7] * y) + m[8]
        iw = np.where(W != 0.0, 32.0 / W, 0.0)
        fx, fy = X * iw, Y * iw
        ok = (np.abs(fx) <= LIMIT) & (np.abs(fy) <= LIMIT)      # False for NaN
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


def warp_batch(src, M, dsize=None, border=BORDER_CONSTANT, border_value=0):
    """warp() per image of src [B,...] with M [B,3,3] -> (dst [B,...], covered [B] int32)."""
    res = [warp(s, m, dsize, border, border_value) for s, m in zip(src, M)]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res], np.int32)


def matrices(sh, sw, dh, dw):
    """name -> 3x3 destination -> source matrix for a dh x dw destination over an sh x sw source."""
    I = np.eye(3)

    def shift(tx, ty):
        return np.array([[1.0, 0, tx], [0, 1.0, ty], [0, 0, 1.0]])

    c, s = np.cos(0.3), np.sin(0.3)
    cx, cy = (sw - 1) / 2.0, (sh - 1) / 2.0
    rot = shift(cx, cy) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ shift(-(dw - 1) / 2.0, -(dh - 1) / 2.0)
    xz = 0.6 * max(dw - 1, 1)                                   # W = 1 - x / xz: zero inside the frame, negative to its right
    persp = np.array([[1.0, 0.1, 0.0], [0.05, 1.0, 0.0], [-1.0 / xz, 0.0, 1.0]])
    nan, inf, zero = I.copy(), I.copy(), np.zeros((3, 3))
    nan[0, 1] = np.nan
    inf[1, 2] = np.inf
    wnan = I.copy(); wnan[2, 0] = np.nan
    return {
        "identity": I, "shift_int": shift(3.0, -2.0), "shift_half": shift(0.5, 0.5), "shift_64th": shift(1.0 / 64, 1.0 / 64),
        "rotation": rot, "perspective": persp, "scale_1e-3": np.diag([1e-3, 1e-3, 1.0]), "scale_1e3": np.diag([1e3, 1e3, 1.0]),
        # fx = 32 (x + t): with t = 2^25 - 2 the columns x = 0, 1, 2 lie at and below 2^30 and x >= 3 beyond it; likewise below zero, and in y
        "limit_pos": shift(2.0 ** 25 - 2.0, 0.0), "limit_neg": shift(-(2.0 ** 25) - 2.0, 0.0), "limit_y": shift(0.0, 2.0 ** 25 - 1.0),
        "nan": nan, "inf": inf, "nan_in_w": wnan, "zero": zero,
    }


SEQUENCES = (((0.004, -0.003, 0.002), (0.003, -0.002, 0.01)), ((0.002, 0.001, 0.0), (0.001, 0.002, 0.03)))
_cache = {}


def sequence(which, h=240, w=320, seed=5, n_frames=12):
    """(gray [n,h,w] uint8, H [n,3,3]): the frames of render_sequence(motion="finite") through the BGR -> gray rule of ofk.h, and per
    frame k the true homography H^k that maps a pixel of frame 0 to frame k - the destination -> source matrix that warps frame k into
    frame 0's view.  Computed once per argument set; callers leave the arrays as they are."""
    key = (which, h, w, seed, n_frames)
    if key not in _cache:
        from of_amd import synth
        v, om = SEQUENCES[which]
        frames, info = synth.render_sequence(h, w, seed, n_frames, v=v, omega=om, motion="finite")
        f = frames.astype(np.uint32)
        gray = ((f[..., 0] * 3735 + f[..., 1] * 19235 + f[..., 2] * 9798 + 16384) >> 15).astype(np.uint8)
        H1 = synth.pixel_homography(v, om, 1.0, (0, 0, 1), info["scaling"], info["cx"], info["cy"], motion="finite")
        H = np.stack([np.linalg.matrix_power(H1, k) for k in range(n_frames)])
        gray.setflags(write=False); H.setflags(write=False)
        _cache[key] = (gray, H)
    return _cache[key]


def stabilised_figures(gray, H, border=BORDER_CONSTANT):
    """Per frame k >= 1: (mean |warp(frame k) - frame 0| over the covered pixels, mean |frame k - frame 0| over the frame, cover)."""
    ref = gray[0].astype(np.int32)
    rows = []
    for k in range(1, len(gray)):
        out, mask = warp_mask(gray[k], H[k], None, border, 0)
        stab = np.abs(out.astype(np.int32) - ref)[mask].mean()
        raw = np.abs(gray[k].astype(np.int32) - ref).mean()
        rows.append((float(stab), float(raw), float(mask.mean())))
    return rows


# ------------------------------------------------------------------------------------------------ the view (ofk.h: ofk_set_stabilise)
STAB_OFF, STAB_ROTATION, STAB_PLANE = 0, 1, 2
NONE, ROTATION_ONLY, FULL = 0, 1, 2
RB_COVER, RB_FINITE = 1, 2
STAB_DOUBLES, STAB_INTS = 48, 4
KEY_SOLVED, KEY_NONE = 0, 2
DEFAULTS = dict(mode=STAB_PLANE, border=BORDER_CONSTANT, border_value=0, min_cover=0.5, chain=1)


def setting(**kw):
    s = dict(DEFAULTS)
    s.update(kw)
    return s


def empty():
    return dict(Bv=np.eye(3), ints=np.zeros(STAB_INTS, np.int32))


def mul3(A, B):
    out = np.zeros((3, 3))
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                out[i, j] = (A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]
    return out


def pixels(A, sc, cx, cy):
    """M = K A K^-1 entry by entry as ofk.h writes it."""
    with np.errstate(all="ignore"):
        f, kx, ky = 1.0 / sc, cx * sc, cy * sc
        P = np.zeros((3, 3))
        for j in range(3):
            P[0, j] = f * A[0, j] + cx * A[2, j]; P[1, j] = f * A[1, j] + cy * A[2, j]; P[2, j] = A[2, j]
        M = np.zeros((3, 3))
        for i in range(3):
            M[i, 0] = P[i, 0] * sc; M[i, 1] = P[i, 1] * sc; M[i, 2] = P[i, 2] - (P[i, 0] * kx + P[i, 1] * ky)
    return M


def pose(R, key_rec, sn, h, w, state=None, normal=None, prev_covered=0, s=None):
    """Rules 1-4 of ofk.h for one stream: R [3,3] the rotation used, key_rec the keyframe's record, sn the sensor row, state
    dict(Bv, ints) of the previous step (None: the identity), prev_covered read where ints[3] != 0.  -> (state, rec [48])."""
    s = setting() if s is None else s
    st = empty() if state is None else state
    R = np.asarray(R, np.float64).reshape(3, 3)
    key_rec, sn = np.asarray(key_rec, np.float64), np.asarray(sn, np.float64)
    T = key_rec[0:3].copy()
    kflag, rekey = int(key_rec[3]), key_rec[9] != 0.0
    n = sn[1:4] if normal is None else np.asarray(normal, np.float64)
    I = np.eye(3)
    with np.errstate(all="ignore"):
        den = sn[0] - ((n[0] * T[0] + n[1] * T[1]) + n[2] * T[2])
        fin = bool(np.isfinite(den) and np.all(np.isfinite(n)) and np.all(np.isfinite(T)) and np.all(np.isfinite(R)))
        flag = ROTATION_ONLY
        if kflag == KEY_NONE:
            flag = NONE
        elif s["mode"] == STAB_PLANE and kflag == KEY_SOLVED and abs(den) >= 1e-12 and fin:
            flag = FULL
        if flag == FULL:
            C = np.array([[(1.0 if i == j else 0.0) + (T[i] * n[j]) / den for j in range(3)] for i in range(3)])
            G = mul3(C, R)
        else:
            G = I.copy() if flag == NONE else R.copy()
        ints = np.asarray(st["ints"], np.int32)
        prev = int(prev_covered) if ints[3] != 0 else -1
        reason = RB_COVER if (s["min_cover"] > 0.0 and prev >= 0 and float(prev) < s["min_cover"] * (float(h) * float(w))) else 0
        B0 = I.copy() if reason else np.asarray(st["Bv"], np.float64).reshape(3, 3)
        A = mul3(G, B0)
        M = pixels(A, sn[19], sn[20], sn[21])
        if not np.all(np.isfinite(M)) and reason == 0:
            reason = RB_FINITE
            B0 = I.copy()
            A = mul3(G, B0)
            M = pixels(A, sn[19], sn[20], sn[21])
    since, rebases, approx = int(ints[0]), int(ints[1]), int(ints[2])
    if reason:
        since, rebases = 0, rebases + 1
    else:
        since += 1
    if rekey and flag != FULL:
        approx += 1
    Bv = (A if s["chain"] else I.copy()) if rekey else B0
    rec = np.zeros(STAB_DOUBLES)
    rec[0:9] = M.ravel(); rec[9:18] = Bv.ravel(); rec[18:27] = R.ravel(); rec[27:30] = T
    rec[30:37] = [flag, reason, since, rebases, approx, 1.0 if rekey else 0.0, prev]
    return dict(Bv=Bv.copy(), ints=np.array([since, rebases, approx, 1], np.int32)), rec


def view_run(gray, mats, h, w, s):
    """The view's bookkeeping over a sequence whose per-step homographies are known: mats[k] maps a pixel of frame 0 to frame k; the
    keyframe is frame 0 throughout (no re-key), G is fed through a unit camera.  -> per step (rec, frame, covered)."""
    sn = np.zeros(28); sn[0] = 1.0; sn[3] = 1.0; sn[19] = 1.0
    key = np.zeros(32)
    state, cov, out = None, 0, []
    for k in range(1, len(gray)):
        state, rec = pose(mats[k], key, sn, h, w, state, prev_covered=cov, s=setting(**dict(s, mode=STAB_ROTATION)))
        frame, cov = warp(gray[k], rec[0:9].reshape(3, 3), None, s["border"], s["border_value"])
        out.append((rec, frame, cov))
    return out


def chain(which, n_frames=12, h=240, w=320, seed=5, corners=150, s=None, key=None):
    """The CPU chain over sequence `which`: the corners of frame 0 through the C oracle's LK and the template restatement, the keyframe
    restatement on the tracks (no re-detection), pose() on its record and the rotation its rule 1 formed, warp() of every frame into
    the view.  The first step finds no keyframe, leaves frame 1 as it is and keys on it: the view is frame 1's, so the figures are
    taken against frame 1 from frame 2 on.  -> dict(rows: per frame k >= 2 (stabilised mean abs diff against frame 1 over the covered
    pixels, raw mean abs diff frame k - frame 1, cover), flags, rebases, approx, keyframes, gain: the smallest raw / stabilised)."""
    import keyframe_reference as K
    import track_template_reference as tr
    from of_amd import synth
    from oracle import image_oracle as io
    s = setting() if s is None else s
    ks = K.setting() if key is None else key
    v, om = SEQUENCES[which]
    frames, info = synth.render_sequence(h, w, seed, n_frames, v=v, omega=om, motion="finite")
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
    ref = gray[1].astype(np.int32)
    state, cov, out = None, 0, dict(rows=[], flags=[], rebases=0)
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
        one["key_xy"] = pad(pts, 2); one["member"][:] = 1
        one["state"] = K.empty(1)["state"]; one["istate"] = np.array([k, n, 0, 0], np.int32)
        _, r1, _, _ = K.step(one, pad(nxt, 2), pad(stt), n, sn, np.zeros(3), False, k, dr_s)
        R_used = K.mul3(K.rotation(sn[4:7]), kst["state"][:9].reshape(3, 3))      # rule 1's product, in front of rule 5
        kst, krec, cnt, _ = K.step(kst, pad(nxt, 2), pad(stt), n, sn, r1[10:13], r1[3] == K.SOLVED, k, ks)
        state, prec = pose(R_used, krec, sn, h, w, state, prev_covered=cov, s=s)
        frame, mask = warp_mask(gray[k + 1], prec[0:9].reshape(3, 3), None, s["border"], s["border_value"])
        cov = int(np.count_nonzero(mask))
        stab = float(np.abs(frame.astype(np.int32) - ref)[mask].mean()) if cov else float("nan")
        raw = float(np.abs(gray[k + 1].astype(np.int32) - ref).mean())
        if k >= 1:
            out["rows"].append((stab, raw, cov / float(h * w)))
        out["flags"].append(int(prec[30]))
        pts = nxt[stt != 0]
    out["rebases"], out["approx"], out["keyframes"] = int(prec[33]), int(prec[34]), int(kst["istate"][2])
    out["gain"] = min(r / st for st, r, _ in out["rows"])
    return out
