"""The perspective warp and the stabilised view per stream on the device (ofk.h: ofk_warp_perspective, ofk_set_stabilise).

(a) k_warp_u8 against its numpy restatement (tests/stabilise_reference.py), bit for bit: frames and covered counts, over sizes from
    1 x 1 to 240 x 320 with a destination that differs from the source, both channel counts, both borders, border values 0 and 200,
    batches of 1, 3 and 65 images with distinct matrices, and the matrices of stabilise_reference.matrices(): rounding ties, a W that
    changes sign inside the frame, |fx| on either side of 2^30, NaN, inf and zero.  The rendered finite-motion sequences warped into
    their first frame's view with the true homographies, at half the CPU figure's smallest gain.
(b) k_stab_pose through ofk_stab_pose against pose(): M, Bv, R, T within 1e-9 of each group's scale (the largest deviation is printed),
    flags, reasons and counts bit for bit; streams without a keyframe, a refused key solve, |d - n.T| below its limit, mode rotation,
    chain 0 and 1, a re-base by cover (and none at exactly min_cover h w) and by a non-finite M, 1, 64 and 65 streams.
(c) Two 240 x 320 streams (the two motions of the issue's table) over 12 frames through ofk_stream_step and ofk_stream_step_fused:
    append and replace re-detection, a JPEG step, held steps, use_imu, the setting switched on in mid-stream, beside the keyframe
    rotation and the keyframe map, max_age = 3 (the view chained over three re-keys).  Every step's record is ofk_stab_pose's on the
    downloads, every frame the warp stage entry's on the downloaded M, every other output of the run the bits of the run with the
    setting off; the device's gain is at least half the CPU chain's.
(d) Refusals: without the keyframe, beside the camera model, beside the rolling shutter; ofk_stab_reset."""
import dataclasses

import numpy as np
import pytest

import keyframe_reference as K
import stabilise_reference as sr
from test_gpu_keyframe import bits, same

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (3, 5), (64, 16), (67, 33), (240, 320))         # (h, w)


@pytest.fixture(scope="module")
def ctx(ofk):
    c = ofk.Context(0, 320, 240, 65, 16, 2)
    yield c
    c.close()


def image(h, w, ch, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, ch) if ch == 3 else (h, w), dtype=np.uint8)


def check(ctx, src, M, dsize, border, bval):
    got, cov = ctx.warp_perspective(src, M, dsize, border, bval)
    want, wcov = sr.warp_batch(src, M, dsize, border, bval)
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = [b for b in range(len(M)) if not np.array_equal(got[b], want[b])]
    assert not bad, (bad, [int(np.count_nonzero(got[b] != want[b])) for b in bad])
    assert np.array_equal(cov, wcov), (cov, wcov)
    return got, cov


# every source size meets a destination of another size (the next in the list) and its own
PAIRS = [(s, SIZES[(i + 1) % len(SIZES)]) for i, s in enumerate(SIZES)] + [(s, s) for s in SIZES]


@pytest.mark.parametrize("ch", (1, 3))
@pytest.mark.parametrize("border,bval", ((sr.BORDER_CONSTANT, 0), (sr.BORDER_CONSTANT, 200), (sr.BORDER_REPLICATE, 0), (sr.BORDER_REPLICATE, 200)))
@pytest.mark.parametrize("ssize,dsize", PAIRS)
def test_every_matrix_bit_for_bit(ctx, ssize, dsize, ch, border, bval):
    """One batch per case: every matrix of matrices() over its own random image."""
    mats = sr.matrices(*ssize, *dsize)
    M = np.stack(list(mats.values()))
    src = np.stack([image(*ssize, ch, 100 + k) for k in range(len(M))])
    got, cov = check(ctx, src, M, dsize, border, bval)
    names = list(mats)
    if ssize == dsize:
        assert np.array_equal(got[names.index("identity")], src[names.index("identity")])
        assert cov[names.index("identity")] == (ssize[0] - 1) * (ssize[1] - 1)
    for name in ("nan", "inf", "nan_in_w"):                       # nothing is ok: the border value everywhere, under either border
        b = names.index(name)
        assert cov[b] == 0
    assert np.all(got[names.index("nan_in_w")] == bval)


@pytest.mark.parametrize("batch", (1, 3, 65))
@pytest.mark.parametrize("ch", (1, 3))
def test_batches_of_distinct_matrices(ctx, batch, ch):
    """Near-rigid motions, one per image, 67 x 33 -> 64 x 16 and 240 x 320 -> 240 x 320 (the stream's case)."""
    rng = np.random.default_rng(7 + batch)
    for ssize, dsize in (((67, 33), (64, 16)), ((240, 320), (240, 320))):
        M = np.empty((batch, 3, 3))
        for b in range(batch):
            a = rng.uniform(-0.2, 0.2)
            M[b] = [[np.cos(a), -np.sin(a), rng.uniform(-8, 8)], [np.sin(a), np.cos(a), rng.uniform(-8, 8)],
                    [rng.uniform(-2e-4, 2e-4), rng.uniform(-2e-4, 2e-4), 1.0]]
        src = np.stack([image(*ssize, ch, 300 + b) for b in range(batch)])
        _, cov = check(ctx, src, M, dsize, sr.BORDER_CONSTANT, 0)
        assert len(set(cov.tolist())) > 1 or batch == 1


def test_single_image_and_cv2_facade(ctx, pkg):
    from of_amd import cv2_hip
    src = image(67, 33, 1, 1)
    M = sr.matrices(67, 33, 64, 16)["rotation"]
    got, cov = ctx.warp_perspective(src, M, (64, 16), "replicate", 0)
    want, wcov = sr.warp(src, M, (64, 16), sr.BORDER_REPLICATE, 0)
    assert np.array_equal(got, want) and cov == wcov and isinstance(cov, int)
    fwd = np.array([[0.9, 0.1, 2.0], [-0.1, 0.9, 1.0], [1e-4, 0.0, 1.0]])       # source -> destination: inverted on the host
    bgr = image(33, 67, 3, 2)
    a = cv2_hip.warpPerspective(bgr, fwd, (40, 30), borderValue=7)
    assert np.array_equal(a, sr.warp(bgr, np.linalg.inv(fwd), (30, 40), sr.BORDER_CONSTANT, 7)[0])
    b = cv2_hip.warpPerspective(bgr, fwd, (40, 30), flags=cv2_hip.INTER_LINEAR | cv2_hip.WARP_INVERSE_MAP, borderMode=cv2_hip.BORDER_REPLICATE)
    assert np.array_equal(b, sr.warp(bgr, fwd, (30, 40), sr.BORDER_REPLICATE, 0)[0])


def test_refusals(ctx, ofk):
    src, M = image(8, 8, 1, 3), np.eye(3)
    for kw in (dict(border=2), dict(border=-1), dict(border_value=256), dict(border_value=-1), dict(dsize=(241, 320))):
        with pytest.raises(ofk.OfkError) as e:
            ctx.warp_perspective(src, M, **kw)
        assert e.value.code == ofk.E_INVALID, kw
    with pytest.raises(ofk.OfkError) as e:                          # more images than the context's batch
        ctx.warp_perspective(np.zeros((66, 4, 4), np.uint8), np.tile(np.eye(3), (66, 1, 1)))
    assert e.value.code == ofk.E_INVALID
    with pytest.raises(ofk.OfkError) as e:                          # a source beyond the context's frame
        ctx.warp_perspective(np.zeros((241, 320), np.uint8), M, (8, 8))
    assert e.value.code == ofk.E_INVALID
    L = ofk.load_library()
    out = np.zeros((8, 8, 2), np.uint8)
    two = np.zeros((8, 8, 2), np.uint8)
    assert L.ofk_warp_perspective(ctx._h, ofk._p(two), 8, 8, 2, ofk._p(M), ofk._p(out), 8, 8, 0, 0, 1, None) == ofk.E_INVALID
    assert L.ofk_warp_perspective(ctx._h, None, 8, 8, 1, ofk._p(M), ofk._p(out), 8, 8, 0, 0, 1, None) == ofk.E_INVALID
    got, cov = ctx.warp_perspective(src, M)                         # and the context still works
    assert np.array_equal(got, src) and cov == 49


@pytest.mark.parametrize("which", (0, 1))
def test_true_homographies_hold_the_ground_still(ctx, pkg, which):
    """The issue's table on the device: frame k warped into frame 0's view with the true homography.  The device's frames and counts
    are the restatement's, so the figures are the CPU's (tests/test_stabilise_reference.py); asserted at half its smallest gain."""
    gray, H = sr.sequence(which)
    got, cov = check(ctx, gray[1:], H[1:], None, sr.BORDER_CONSTANT, 0)
    ref = gray[0].astype(np.int32)
    for k in range(1, len(gray)):
        mask = sr.warp_mask(gray[k], H[k])[1]
        assert cov[k - 1] == np.count_nonzero(mask)
        stab = np.abs(got[k - 1].astype(np.int32) - ref)[mask].mean()
        raw = np.abs(gray[k].astype(np.int32) - ref).mean()
        assert stab * 5.0 <= raw, (k, stab, raw)


# ------------------------------------------------------------------------------------------------ the view's pose (k_stab_pose)
DEV = dict(M=0.0, Bv=0.0, R=0.0, T=0.0)                           # the largest deviations met, in units of the group's scale
TOL = 1e-9                                                       # the project's bound for f64 records against their restatement
GROUPS = (("M", 0, 9), ("Bv", 9, 18), ("R", 18, 27), ("T", 27, 30))
EXACT = list(range(30, 48))
KINDS = ("full", "full-rekey", "none", "unsolved", "unsolved-rekey", "den", "cover", "cover-exact", "nan-bv", "inf-bv", "nan-r", "first")


def device_stab(ofk, s):
    return ofk.Stabilise(s["mode"], s["border"], s["border_value"], s["min_cover"], s["chain"])


def pose_case(rng, kind, h, w):
    """One stream's inputs: R, key_rec, sensor row, normal, state, prev_covered."""
    R = K.rotation(rng.uniform(-0.05, 0.05, 3))
    n = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), 1.0]); n /= np.linalg.norm(n)
    d = rng.uniform(0.5, 2.0)
    T = rng.uniform(-0.05, 0.05, 3)
    key = np.zeros(32)
    key[0:3] = T; key[3] = 0.0; key[9] = 0.0
    sn = np.zeros(28)
    sn[0] = d; sn[1:4] = n; sn[19] = 1.0 / max(h, w); sn[20] = w / 2.0; sn[21] = h / 2.0
    Bv = mul_near(rng)
    ints = np.array([int(rng.integers(0, 9)), int(rng.integers(0, 5)), int(rng.integers(0, 5)), 1], np.int32)
    prev = int(0.9 * h * w)
    if kind in ("full-rekey", "unsolved-rekey"):
        key[9] = float(rng.integers(1, 6))
    if kind == "none":
        key[0:3] = 0.0; key[3] = 2.0; key[9] = 1.0
    if kind in ("unsolved", "unsolved-rekey"):
        key[0:3] = 0.0; key[3] = 1.0
    if kind == "den":                                            # the plane through the camera: d - n.T below its limit
        key[0:3] = n * d * (1.0 + 1e-14)
    if kind == "cover":
        prev = int(0.3 * h * w)
    if kind == "cover-exact":                                    # exactly min_cover h w: not below it
        prev = int(0.5 * h * w)
    if kind == "nan-bv":
        Bv[1, 2] = np.nan
    if kind == "inf-bv":
        Bv[0, 0] = np.inf
    if kind == "nan-r":
        R[2, 1] = np.nan
    if kind == "first":
        Bv = np.eye(3); ints[:] = 0; prev = 123
    return dict(R=R, key=key, sn=sn, normal=None, state=dict(Bv=Bv, ints=ints), prev=prev)


def mul_near(rng):
    B = K.rotation(rng.uniform(-0.03, 0.03, 3))
    B[:, 2] += rng.uniform(-0.02, 0.02, 3)
    return B


def same_pose(got_state, got_rec, want_state, want_rec, tag):
    assert np.array_equal(bits(got_rec[EXACT]), bits(want_rec[EXACT])), (tag, got_rec[30:37], want_rec[30:37])
    assert np.array_equal(got_state["ints"], want_state["ints"]), (tag, got_state["ints"], want_state["ints"])
    for name, lo, hi in GROUPS:
        g, wv = got_rec[lo:hi], want_rec[lo:hi]
        f = np.isfinite(wv)
        assert np.array_equal(np.isnan(g), np.isnan(wv)) and np.array_equal(g[np.isinf(wv)], wv[np.isinf(wv)]), (tag, name, g, wv)
        if f.any():
            scale = max(np.abs(wv[f]).max(), 1e-300)
            err = float((np.abs(g[f] - wv[f]) / scale).max())
            DEV[name] = max(DEV[name], err)
            assert err <= TOL, (tag, name, err, g, wv)
    assert np.array_equal(bits(got_state["Bv"].ravel()), bits(got_rec[9:18])), tag


@pytest.mark.parametrize("mode,chain", ((sr.STAB_PLANE, 1), (sr.STAB_PLANE, 0), (sr.STAB_ROTATION, 1)))
@pytest.mark.parametrize("streams", (1, 64, 65))
def test_pose_against_the_restatement(ctx, ofk, streams, mode, chain):
    h, w = 240, 320
    rng = np.random.default_rng(11 * streams + mode + chain)
    s = sr.setting(mode=mode, chain=chain)
    kinds = [KINDS[(b + streams) % len(KINDS)] for b in range(streams)]
    cases = [pose_case(rng, k, h, w) for k in kinds]
    if streams > 1:
        cases[1]["normal"] = np.array([0.05, -0.02, 0.99])       # one stream's normal from elsewhere (the IMU state's under use_imu)
    normal = None
    if streams > 1:
        normal = np.stack([c["sn"][1:4] if c["normal"] is None else c["normal"] for c in cases])
    state = dict(Bv=np.stack([c["state"]["Bv"] for c in cases]), ints=np.stack([c["state"]["ints"] for c in cases]))
    out, rec = ctx.stab_pose(np.stack([c["R"] for c in cases]), np.stack([c["key"] for c in cases]), np.stack([c["sn"] for c in cases]), h, w,
                             state=state, normal=normal, prev_covered=[c["prev"] for c in cases], stabilise=device_stab(ofk, s))
    seen = set()
    for b, c in enumerate(cases):
        ws, wr = sr.pose(c["R"], c["key"], c["sn"], h, w, c["state"], None if normal is None else normal[b], c["prev"], s)
        same_pose(dict(Bv=out["Bv"][b], ints=out["ints"][b]), rec[b], ws, wr, (streams, mode, chain, b, kinds[b]))
        seen.add((kinds[b], int(wr[30]), int(wr[31])))
    print("pose: largest deviation in units of the group's scale", DEV)
    if streams >= 64 and mode == sr.STAB_PLANE:                  # every branch was met
        assert {("full", sr.FULL, 0), ("none", sr.NONE, 0), ("unsolved", sr.ROTATION_ONLY, 0), ("den", sr.ROTATION_ONLY, 0), ("cover", sr.FULL, sr.RB_COVER),
                ("cover-exact", sr.FULL, 0), ("nan-bv", sr.FULL, sr.RB_FINITE), ("inf-bv", sr.FULL, sr.RB_FINITE),
                ("nan-r", sr.ROTATION_ONLY, sr.RB_FINITE)} <= seen, seen
    if mode == sr.STAB_ROTATION and streams >= 64:
        assert all(f != sr.FULL for _, f, _ in seen)


def test_pose_python_stage_entries_and_refusals(ctx, pkg, ofk):
    from of_amd import simulation, velocity_node
    rng = np.random.default_rng(3)
    c = pose_case(rng, "full-rekey", 240, 320)
    for mod in (velocity_node, simulation):
        state, want = None, None
        for t in range(3):
            state, rec = mod.stabilise_step(c["R"], c["key"], c["sn"], 240, 320, state=state, prev_covered=None if t == 0 else 70000, min_cover=0.4)
            if want is not None:
                want["ints"][3] = 1
            want, wrec = sr.pose(c["R"], c["key"], c["sn"], 240, 320, want, None, 70000, sr.setting(min_cover=0.4))
            same_pose(state, rec, want, wrec, (mod.__name__, t))
    args = (c["R"][None], c["key"][None], c["sn"][None], 240, 320)
    with pytest.raises(ofk.OfkError):
        ctx.stab_pose(*args, stabilise=ofk.stabilise_setting(False))
    for bad in (ofk.Stabilise(3, 0, 0, 0.5, 1), ofk.Stabilise(2, 2, 0, 0.5, 1), ofk.Stabilise(2, 0, 256, 0.5, 1), ofk.Stabilise(2, 0, 0, 1.0, 1),
                ofk.Stabilise(2, 0, 0, float("nan"), 1), ofk.Stabilise(2, 0, 0, 0.5, 2)):
        with pytest.raises(ofk.OfkError) as e:
            ctx.stab_pose(*args, stabilise=bad)
        assert e.value.code == ofk.E_INVALID


# ------------------------------------------------------------------------------------------------ the view in the stream steps
SH, SW, SNF, NB = 240, 320, 12, 2
SMC, SMC_BEGIN, SRADIUS = 150, 120, 8
CHAIN_GAIN = 20.3                                                # tests/test_stabilise_reference.py: the CPU chain's smallest gain
_seq = {}


def stream_frames(pkg):
    """Two streams, one per motion of the issue's table: BGR frames [2, 12, 240, 320, 3] and per stream the sensor row of every step."""
    if "f" not in _seq:
        from of_amd import synth
        import of_amd.ofk as ofk
        frames, sensors = [], []
        for v, om in sr.SEQUENCES:
            f, info = synth.render_sequence(SH, SW, 5, SNF, v=v, omega=om, motion="finite")
            frames.append(f)
            sensors.append(ofk.make_sensors(1, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"],
                                            v_prior=info["v"])[0])
        _seq["f"] = (np.stack(frames), np.stack(sensors))
    return _seq["f"]


def stab_cfg(kind, stab, max_age=3, **kw):
    from of_amd.pipeline import PipelineConfig
    extra = {}
    if kind == "rot":
        extra = dict(keyframe_rotation=True)
    if kind == "map":
        extra = dict(track_depth=True, keyframe_map=True)
    return PipelineConfig(max_corners=SMC, quality=0.01, min_distance=10, block_size=3, win=15, max_level=3, max_count=30, eps=0.01, min_eig_thr=1e-4,
                          track_table=True, finite_motion=True, keyframe=_keyframe(max_age), stabilise=stab, **extra, **kw)


def _keyframe(max_age):
    import of_amd.ofk as ofk
    return ofk.keyframe_setting(max_age=max_age)


def run_view(pkg, ofk, kind, stab_on=True, on_from=1, jpeg_step=None, s=None, max_age=3, check=True):
    """kind: "plain" (ofk_stream_step, append re-detection) | "fused" | "imu" (use_imu) | "replace" (the replace re-detection) | "hold" (one
    stream, steps 4 and 5 held) | "rot" (the keyframe rotation on) | "map" (the keyframe map on).  With the setting on (from step on_from
    on) every step's M is ofk_stab_pose's on the downloads, every frame the warp stage entry's on the downloaded M, every record the
    restatement's within TOL.  -> (everything else the calls returned, per step (rec, covered, frames))."""
    from of_amd.pipeline import FlowStream, FusionConfig
    from test_gpu_keyframe import jpeg_of
    s = sr.setting() if s is None else s
    frames, sensors = stream_frames(pkg)
    nb = 1 if kind == "hold" else NB
    frames, sensors = frames[:nb], sensors[:nb]
    fused = kind != "plain"
    late = stab_on and on_from > 1
    cfg = stab_cfg(kind, device_stab(ofk, s) if stab_on and not late else None, max_age)
    fusion = FusionConfig(use_imu=kind == "imu", redetect_replace=kind == "replace", hold_on_skip=kind == "hold")
    mf = SMC - 10 if kind == "replace" else SMC if kind == "plain" else 0
    fs = FlowStream(SW, SH, batch=nb, cfg=cfg, min_features=mf, mask_radius=SRADIUS, fusion=fusion if fused else None)
    ctx, side = fs.ctx, ofk.Context(0, SW, SH, nb, 16, 1)
    out, views, state, prev_cov, held, rekeys, events = [], [], None, None, 0, 0, 0
    try:
        ctx.imu_reset(nb)
        tracks, counts = ctx.stream_begin(frames[:, 0], dataclasses.replace(cfg, max_corners=SMC_BEGIN if kind == "plain" else SMC).to_params())
        for t in range(1, SNF):
            if late and t == on_from:
                ctx.set_stabilise(device_stab(ofk, s))
            on = stab_on and t >= on_from
            before = counts.copy()
            if not fused:
                if t == jpeg_step:
                    rec, tracks, counts = ctx.stream_step_jpeg(jpeg_of(frames[:, t]), sensors, cfg.to_params(), mf, SRADIUS)
                else:
                    rec, tracks, counts = ctx.stream_step(frames[:, t], sensors, cfg.to_params(), mf, SRADIUS)
                fz = None
            else:
                fst = fusion.to_struct()
                if kind == "hold" and t in (4, 5):
                    fst.min_solve = 10 ** 6                      # more points than there are: not solved, held
                rec, fz, tracks, counts = ctx.stream_step_fused(frames[:, t], sensors, cfg.to_params(), fst, mf, SRADIUS)
            hold = kind == "hold" and rec[0, 15] == 0
            kd = ctx.keyframe_download(nb, SMC)
            row = (rec.copy(), tracks.copy(), counts.copy(), ctx.track_table_download(nb, SMC), {k: kd[k] for k in ("R_acc", "rec")}) + (() if fz is None else (fz.copy(),))
            if kind == "rot":
                row += (ctx.keyframe_rotation_download(nb),)
            if kind == "map":
                row += (ctx.keyframe_map_download(nb, SMC)["rec"], ctx.track_depth_download(nb, SMC)["rec"])
            out.append(row)
            if not on:
                continue
            d = ctx.stab_download(nb, SH, SW)
            if hold:                                             # a held step launches nothing: state, record, count and frame stay
                held += 1
                assert np.array_equal(bits(d["rec"]), bits(views[-1][0])) and np.array_equal(d["covered"], views[-1][1]) and np.array_equal(d["frames"], views[-1][2])
                continue
            views.append((d["rec"].copy(), d["covered"].copy(), d["frames"].copy()))
            if not check:
                continue
            R_used = d["rec"][:, 18:27].reshape(nb, 3, 3)
            if kind == "rot":
                assert np.array_equal(bits(R_used.reshape(nb, 9)), bits(row[-1][:, 4:13])), (kind, t, "R is the rotation record's")
            for b in range(nb):
                if kd["rec"][b, 9] == 0 and kind != "rot":       # no re-key: rule 1's product is what the state holds behind the step
                    assert np.array_equal(bits(R_used[b]), bits(kd["R_acc"][b])), (kind, t, b, "R is rule 1's product")
            assert np.array_equal(bits(d["rec"][:, 27:30]), bits(kd["rec"][:, 0:3])), (kind, t, "T is the keyframe record's")
            replaced = [b for b in range(nb) if kind == "replace" and before[b] <= mf and SMC - before[b] > 0]
            for b in replaced:                                   # k_stab_clear beside k_keyframe_replace: the view starts over, the counts stay
                if state is not None:
                    state["Bv"][b] = np.eye(3)
            normal = ctx.imu_state(nb)[0][:, 15:18] if kind == "imu" else None
            pc = np.zeros(nb, np.int32) if prev_cov is None else prev_cov
            got_state, got_rec = side.stab_pose(R_used, kd["rec"], sensors, SH, SW, state=state, normal=normal, prev_covered=pc, stabilise=device_stab(ofk, s))
            assert np.array_equal(bits(got_rec), bits(d["rec"])), (kind, t, "the step's record is ofk_stab_pose's on the downloads", got_rec, d["rec"])
            for b in range(nb):
                st_b = None if state is None else dict(Bv=state["Bv"][b], ints=state["ints"][b])
                ws, wr = sr.pose(R_used[b], kd["rec"][b], sensors[b], SH, SW, st_b, None if normal is None else normal[b], int(pc[b]), s)
                same_pose(dict(Bv=got_state["Bv"][b], ints=got_state["ints"][b]), d["rec"][b], ws, wr, (kind, t, b))
            state, prev_cov = got_state, d["covered"].copy()
            gray = np.stack([ctx.resident_pyramid(0, b, SH, SW, 0)[0] for b in range(nb)])       # the step's new frame, as the warp read it
            wf, wc = side.warp_perspective(gray, d["rec"][:, 0:9].reshape(nb, 3, 3), None, s["border"], s["border_value"])
            assert np.array_equal(wf, d["frames"]) and np.array_equal(wc, d["covered"]), (kind, t, "the frame is the warp stage entry's on the downloaded M")
            rekeys += int((kd["rec"][:, 9] != 0).sum())
            for b in replaced:                                   # no keyframe: the new frame goes through as it is
                assert d["rec"][b, 30] == sr.NONE and np.array_equal(d["frames"][b], gray[b]), (kind, t, b)
            events += len(replaced)
        if stab_on:
            sv = fs.stabilised()
            assert np.array_equal(bits(sv["rec"]), bits(views[-1][0])) and np.array_equal(sv["frames"], views[-1][2])
            assert np.array_equal(sv["M"].reshape(nb, 9), views[-1][0][:, 0:9]) and np.array_equal(sv["covered"], views[-1][1])
            ptr, stride = ctx.stab_frames()
            assert ptr and stride >= SH * SW and stride % 256 == 0
            print(kind, "flags", [int(v[0][0, 30]) for v in views], "re-bases", views[-1][0][:, 33], "approx", views[-1][0][:, 34], "re-keys", rekeys, "held", held,
                  "deviation", DEV)
            assert kind != "hold" or held >= 2
            assert kind != "replace" or events >= 1 or not check
    finally:
        fs.close(); side.close()
    return out, views


def gains(views, frames_gray, first=1):
    """Per stream the smallest raw / stabilised mean abs diff against the view's own reference (the first output frame, left as it was)."""
    res = []
    for b in range(frames_gray.shape[0]):
        ref = views[0][2][b].astype(np.int32)
        g = []
        for k, (rec, cov, fr) in enumerate(views[1:], first + 1):
            M = rec[b, 0:9].reshape(3, 3)
            mask = sr.warp_mask(frames_gray[b, k], M)[1]
            stab = np.abs(fr[b].astype(np.int32) - ref)[mask].mean()
            raw = np.abs(frames_gray[b, k].astype(np.int32) - ref).mean()
            g.append(raw / stab)
        res.append(min(g))
    return res


def test_fused_steps_chain_the_view_over_three_rekeys_and_hold_the_ground_still(pkg, ofk):
    """ofk_stream_step_fused, no re-detection (the streams begin full), max_age = 3: the view is chained over three re-keys and the
    device's gain is at least half the CPU chain's.  Measured on the device: 20.3 and 26.6 for the two streams (CPU chain 20.3 and 24.5)."""
    on, views = run_view(pkg, ofk, "fused")
    off, _ = run_view(pkg, ofk, "fused", stab_on=False)
    same(on, off, "fused: the setting on against off")
    frames, _ = stream_frames(pkg)
    side = ofk.Context(0, SW, SH, SNF, 16, 1)
    try:
        gray = np.stack([side.gray_bgr8(frames[b]) for b in range(NB)])
    finally:
        side.close()
    assert np.array_equal(views[0][2], gray[:, 1])               # the first step finds no keyframe: the frame goes through as it is
    assert np.all(views[-1][0][:, 30] == sr.FULL) and np.all(views[-1][0][:, 33] == 0)
    keyframes = [int(np.sum([v[0][b, 35] for v in views])) for b in range(NB)]
    assert min(keyframes) >= 3, keyframes
    g = gains(views, gray)
    print("device gain per stream", g, "CPU chain", CHAIN_GAIN)
    assert min(g) >= CHAIN_GAIN / 2.0, g


def test_plain_step_with_append_redetection_and_a_jpeg_step(pkg, ofk):
    pytest.importorskip("PIL.Image")
    on, _ = run_view(pkg, ofk, "plain", jpeg_step=3)
    off, _ = run_view(pkg, ofk, "plain", stab_on=False, jpeg_step=3)
    same(on, off, "plain: the setting on against off")


def test_switched_on_in_mid_stream(pkg, ofk):
    on, views = run_view(pkg, ofk, "plain", on_from=4)
    off, _ = run_view(pkg, ofk, "plain", stab_on=False)
    same(on, off, "plain: switched on at step 4 against off")
    assert len(views) == SNF - 4 and views[0][0][0, 32] == 1 and views[0][0][0, 36] == -1      # the view began with that step


@pytest.mark.parametrize("kind", ("imu", "replace", "hold", "rot", "map"))
def test_fused_steps_on_against_off(pkg, ofk, kind):
    on, _ = run_view(pkg, ofk, kind)
    off, _ = run_view(pkg, ofk, kind, stab_on=False)
    same(on, off, (kind, "the setting on against off"))


@pytest.mark.parametrize("name,kw", (("chain0", dict(chain=0)), ("rotation", dict(mode=sr.STAB_ROTATION)), ("replicate", dict(border=sr.BORDER_REPLICATE, border_value=200)),
                                     ("cover", dict(min_cover=0.97))))
def test_settings_in_the_stream(pkg, ofk, name, kw):
    _, views = run_view(pkg, ofk, "fused", s=sr.setting(**kw))
    rec = views[-1][0]
    if name == "chain0":                                         # the view jumps to every new keyframe: Bv is the identity behind a re-key
        assert any(v[0][0, 35] == 1 and np.array_equal(v[0][0, 9:18], np.eye(3).ravel()) for v in views[1:])
    if name == "rotation":
        assert all(np.all(v[0][:, 30] != sr.FULL) for v in views) and np.all(rec[:, 34] >= 3)
    if name == "cover":                                          # the frame leaves the view: re-based on the current keyframe
        assert np.all(rec[:, 33] >= 1) and any(np.any(v[0][:, 31] == sr.RB_COVER) for v in views)


def test_stream_refusals_and_reset(pkg, ofk):
    from of_amd.pipeline import CameraModel
    frames, sensors = stream_frames(pkg)
    cfg = stab_cfg("fused", None)
    ctx = ofk.Context(0, SW, SH, NB, SMC, cfg.max_level)
    try:
        ctx.set_track_table(ofk.track_table_setting())
        ctx.set_stabilise(ofk.stabilise_setting())
        ctx.stream_begin(frames[:, 0], cfg.to_params())
        step = lambda t=1: ctx.stream_step(frames[:, t], sensors, cfg.to_params(), 0, SRADIUS)

        def refused(name):
            with pytest.raises(ofk.OfkError) as e:
                step()
            assert e.value.code == ofk.E_INVALID and name in str(e.value), (name, str(e.value))
            with pytest.raises(ofk.OfkError):                      # refused before any launch: nothing has stepped with the setting on
                ctx.stab_download(NB, SH, SW)
        refused("ofk_set_keyframe")
        ctx.set_keyframe(ofk.keyframe_setting(max_age=1))        # a re-key with every step: the view is chained from the first one on
        ctx.set_camera(CameraModel(fx=320.0, fy=320.0, cx=160.0, cy=120.0, k=(-0.1, 0.01, 0, 0)).setting())
        refused("ofk_set_camera")
        ctx.set_camera(None)
        ctx.set_rolling_shutter(ofk.rshutter_setting("flow", readout=0.6, anchor=0.4))
        refused("ofk_set_rolling_shutter")
        ctx.set_rolling_shutter(None)
        with pytest.raises(ofk.OfkError):
            ctx.stab_frames()
        for t in (1, 2, 3):
            step(t)
        d = ctx.stab_download(NB, SH, SW)
        assert np.all(d["rec"][:, 32] == 3) and not np.array_equal(d["rec"][0, 9:18], np.eye(3).ravel())
        ctx.stab_reset(1)
        with pytest.raises(ofk.OfkError):
            ctx.stab_reset(NB)
        r = ctx.stab_download(NB, SH, SW, frames=False)["rec"]
        assert np.array_equal(bits(r[0]), bits(d["rec"][0])) and np.array_equal(r[1, 9:18], np.eye(3).ravel()) and r[1, 32] == 0 and r[1, 36] == -1
        step(4)
        r = ctx.stab_download(NB, SH, SW, frames=False)["rec"]
        assert r[0, 32] == 4 and r[1, 32] == 1 and r[1, 36] == -1
    finally:
        ctx.close()
