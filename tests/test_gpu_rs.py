"""The rolling shutter on the device (include/ofk.h: ofk_set_rolling_shutter) against tests/rs_reference.py.

Stage entry: flow mode bit for bit (compared as uint32), gyro mode within one float32 ulp (sin and cos come from two math libraries);
slots beyond counts keep a sentinel; the fallback rule; readout 0 returns the input bits.  Where a result is not a number only that
is compared: IEEE 754 leaves the sign and payload of a NaN an operation creates to the implementation.
Resident chains: every check is a composition of stage entries - the points the solve saw are ofk_rs_correct_points of the downloaded
raw points (of ofk_undistort_points of them with a camera), the records are the reference solve of those points, and everything that
lives in the image is bit-identical to a run with the setting off.  The stream steps are also held, step by step, to
stream_oracle.NodeLoop with the solver fed from the corrected points (rs_reference.rs_loop)."""
import numpy as np
import pytest

import batch_oracle as BO
import cov_reference as cr
import rs_reference as R
from point_stage_helpers import ROBUST, SENTINEL, assert_image_side_identical, assert_plain_records, bits, robust_reference, same_points
from rs_scene import (B, COV, COVD, FEAS_T, GATE, H, MIN_FEAT, NB, NSTEPS, PAIR_CAM, RADIUS, SEED, SH, SW, W, as_struct, pair_batch, pair_cfg,
                      stream_setup)
from stream_oracle import feasibility_solve, plain_solve

pytestmark = pytest.mark.gpu


def ulp_of(mode):
    return 0 if mode == R.FLOW else 1


@pytest.fixture(scope="module")
def sctx(ofk):
    c = ofk.Context(0, 64, 48, 3, 300, 2)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------- the stage entry
def stage_points(rows, seed):
    """(raw_prev, raw_next, ideal_prev, ideal_next [3,300,2] f32, sensors [3,28]) over a 1280-wide frame of `rows` rows and a border
    around it; image 1 has omega = 0 (theta^2 < 1e-16), and the first points of image 2 are placed to hit the fallback."""
    rng = np.random.default_rng(seed)
    p0 = np.stack([rng.uniform(-60, 1340, (3, 300)), rng.uniform(-0.06 * rows, 1.06 * rows, (3, 300))], -1)
    p1 = p0 + np.stack([rng.uniform(-60, 60, (3, 300)), rng.uniform(-0.08 * rows, 0.08 * rows, (3, 300))], -1)
    p0, p1 = p0.astype(np.float32), p1.astype(np.float32)
    p0[2, 0] = (100.0, 0.95 * rows); p1[2, 0] = (110.0, 0.05 * rows)        # readout 0.9: span 0.19, readout -0.5: 1.45
    p0[2, 1] = (100.0, 0.05 * rows); p1[2, 1] = (110.0, 1.3 * rows)         # readout -0.5: span 0.375
    p1[2, 2] = (np.nan, 0.5 * rows); p1[2, 3] = (300.0, np.nan); p1[2, 4] = (1e7, 0.4 * rows); p1[2, 5] = (np.inf, 0.3 * rows)
    p1[2, 6] = (200.0, -1e7)                                                # the row itself is garbage: span is
    i0 = (p0.astype(np.float64) * 1.013 + (3.25, -2.5)).astype(np.float32)  # some other image the positions live in
    i1 = (p1.astype(np.float64) * 1.013 + (3.25, -2.5)).astype(np.float32)
    sn = np.zeros((3, 28))
    for b, om in enumerate(((0.02, -0.03, 0.15), (0.0, 0.0, 0.0), (-0.004, 0.003, -0.05))):
        sn[b] = R.sensor_row(dict(omega=om), (1e-3, 1.25e-3, 9e-4)[b], (640.0, 652.3, 600.0)[b], 0.5 * rows + b)
    return p0, p1, i0, i1, sn


@pytest.mark.parametrize("mode", [R.FLOW, R.GYRO], ids=["flow", "gyro"])
@pytest.mark.parametrize("rows", [960, 7])
def test_stage_entry_against_the_restatement(ofk, sctx, mode, rows):
    p0, p1, i0, i1, sn = stage_points(rows, 10 + rows)
    counts = (0, 257, 300)
    seen_fallback = 0
    for readout in (0.9, -0.5, 0.0):
        for anchor in (0.0, 0.5, 1.0):
            for ideal in (False, True):
                rs = R.rshutter(mode, readout, anchor, rows, omega_gain=1.0 if anchor != 1.0 else -0.5)
                kw = dict(ideal_prev=i0, ideal_next=i1) if ideal else {}
                a, b = sctx.rs_correct_points(as_struct(ofk, rs), p0, p1, counts, sensors=sn, out=(np.full(p0.shape, SENTINEL), np.full(p0.shape, SENTINEL)), **kw)
                ra, rb, good = R.correct_points(rs, p0, p1, sensors=sn, full=True, **kw)
                tag = (mode, rows, readout, anchor, ideal)
                for i, n in enumerate(counts):
                    assert same_points(a[i, :n], ra[i, :n], ulp_of(mode)) and same_points(b[i, :n], rb[i, :n], ulp_of(mode)), (tag, i)
                    assert np.all(a[i, n:] == SENTINEL) and np.all(b[i, n:] == SENTINEL), (tag, i)
                q0, q1 = (i0, i1) if ideal else (p0, p1)
                bad = ~good[2, :7]
                # not a number and infinity always; 1e7 wherever a result stays beyond 1e6 (flow mode: always); the two spans below 0.5
                assert bad[[2, 3, 5]].all() and (mode == R.GYRO or bad[4]) and (readout == 0.0 or bad[0] == (readout > 0) and bad[1] == (readout < 0)), (tag, bad)
                assert np.array_equal(bits(a[2, :7][bad]), bits(q0[2, :7][bad])) and np.array_equal(bits(b[2, :7][bad]), bits(q1[2, :7][bad])), tag
                seen_fallback += int(bad.sum())
                if readout == 0.0:                               # nothing to undo: the input bits
                    for i, n in enumerate(counts):
                        assert np.array_equal(bits(a[i, :n]), bits(q0[i, :n])) and np.array_equal(bits(b[i, :n]), bits(q1[i, :n])), (tag, i)
                else:
                    assert np.abs(a[1, 10:257] - q0[1, 10:257]).max() > 0.01, tag
    assert seen_fallback > 0
    # flow mode needs no sensors; gyro mode with scaling 0 is the fallback for the whole image
    rs = R.rshutter(mode, 0.9, 0.5, rows)
    if mode == R.FLOW:
        a, b = sctx.rs_correct_points(as_struct(ofk, rs), p0, p1)
        ra, rb = R.correct_points(rs, p0, p1)
        assert same_points(a, ra) and same_points(b, rb)
    else:
        s0 = sn.copy(); s0[0, 19] = 0.0
        a, b = sctx.rs_correct_points(as_struct(ofk, rs), p0, p1, sensors=s0)
        ra, rb = R.correct_points(rs, p0, p1, sensors=s0)
        assert np.array_equal(bits(a[0]), bits(p0[0])) and np.array_equal(bits(b[0]), bits(p1[0]))
        assert same_points(a, ra, 1) and same_points(b, rb, 1)


@pytest.mark.parametrize("mode", [R.FLOW, R.GYRO], ids=["flow", "gyro"])
def test_stage_entry_small_batches(ofk, sctx, mode):
    """One point; counts 255 / 256 at a stride of 256 (one block, with and without an idle thread)."""
    p0, p1, _, _, sn = stage_points(960, 77)
    rs = R.rshutter(mode, -0.9, 0.25, 960, omega_gain=2.0)
    a, b = sctx.rs_correct_points(as_struct(ofk, rs), p0[:1, :1], p1[:1, :1], sensors=sn[:1])
    ra, rb = R.correct_points(rs, p0[:1, :1], p1[:1, :1], sensors=sn[:1])
    assert a.shape == (1, 1, 2) and same_points(a, ra, ulp_of(mode)) and same_points(b, rb, ulp_of(mode)) and not np.array_equal(a, p0[:1, :1])
    a, b = sctx.rs_correct_points(as_struct(ofk, rs), p0[0, :3], p1[0, :3], sensors=sn[:1])
    assert a.shape == (3, 2) and same_points(a, R.correct_points(rs, p0[0, :3], p1[0, :3], sensors=sn[:1])[0], ulp_of(mode))
    q0, q1 = p0[:2, :256], p1[:2, :256]
    a, b = sctx.rs_correct_points(as_struct(ofk, rs), q0, q1, (255, 256), sensors=sn[:2], out=(np.full(q0.shape, SENTINEL), np.full(q0.shape, SENTINEL)))
    ra, rb = R.correct_points(rs, q0, q1, sensors=sn[:2])
    assert same_points(a[0, :255], ra[0, :255], ulp_of(mode)) and same_points(b[1], rb[1], ulp_of(mode)) and same_points(a[1], ra[1], ulp_of(mode))
    assert np.all(a[0, 255] == SENTINEL) and np.all(b[0, 255] == SENTINEL)


# ---------------------------------------------------------------------------------------------------- frame pairs


def corrected_of_download(ctx, ofk, rs, out, sensors, tag, camera=None):
    """ofk_rs_download == ofk_rs_correct_points of the downloaded raw points (of ofk_undistort_points of them with a camera) == the
    numpy restatement: flow mode bit for bit, gyro mode within one ulp, up to counts.  rs: the reference's dict with rows > 0."""
    nb = len(out["counts"])
    m = as_struct(ofk, rs)
    pu, nu = ctx.rs_download(nb)
    kw = {}
    if camera is not None:
        kw = dict(ideal_prev=ctx.undistort_points(camera, out["prev_pts"], out["counts"]), ideal_next=ctx.undistort_points(camera, out["next_pts"], out["counts"]))
    sp, sn = ctx.rs_correct_points(m, out["prev_pts"], out["next_pts"], out["counts"], sensors=sensors, **kw)
    rp, rn = R.correct_points(rs, out["prev_pts"], out["next_pts"], sensors=sensors, **kw)
    moved = 0.0
    for b in range(nb):
        n = int(out["counts"][b])
        assert n > 8, (tag, b, n)
        assert np.array_equal(bits(pu[b, :n]), bits(sp[b, :n])) and np.array_equal(bits(nu[b, :n]), bits(sn[b, :n])), (tag, b)     # one kernel, twice
        assert same_points(pu[b, :n], rp[b, :n], ulp_of(rs["mode"])) and same_points(nu[b, :n], rn[b, :n], ulp_of(rs["mode"])), (tag, b)
        ok = out["status"][b, :n] == 1
        moved = max(moved, float(np.abs(nu[b, :n][ok] - (kw["ideal_next"] if kw else out["next_pts"])[b, :n][ok]).max()))
    assert moved > 0.01, (tag, moved)                            # the correction is not the identity on this scene
    return pu, nu


@pytest.mark.parametrize("streams,overlap,mode", [(1, False, "gyro"), (1, True, "flow"), (2, False, "flow"), (2, True, "gyro")])
def test_pairs_run_is_a_composition_of_stage_entries(pkg, ofk, streams, overlap, mode):
    from of_amd.pipeline import FlowPipeline, RollingShutter
    prev, nxt, sensors = pair_batch(pkg, ofk)
    rsm = RollingShutter(readout=0.9, mode=mode, anchor=0.5)     # rows None: the frame height of the run
    rs = R.rshutter(ofk.RS_MODES[mode], 0.9, 0.5, H)
    tag = (streams, overlap, mode)
    pipe = FlowPipeline(W, H, B, pair_cfg(), streams=streams)
    try:
        pipe.ctx.set_overlap(overlap)
        pipe.upload(prev, nxt, sensors)
        never = pipe.run()
        with pytest.raises(ofk.OfkError):
            pipe.ctx.rs_download(B)
        pipe.ctx.set_rolling_shutter(rsm.setting())
        assert pipe.ctx.get_rolling_shutter().rows == 0
        on = pipe.run()
        pu, nu = corrected_of_download(pipe.ctx, ofk, rs, on, sensors, tag)
        ip, inx = pipe.ideal_points()
        assert np.array_equal(bits(ip), bits(pu)) and np.array_equal(bits(inx), bits(nu))
        with pytest.raises(ofk.OfkError):                        # no run with the camera on: its download keeps its contract
            pipe.ctx.camera_download(B)
        again = pipe.run()                                       # the slices free-run over consecutive calls
        pipe.ctx.set_rolling_shutter(None)
        off = pipe.run()
    finally:
        pipe.close()
    assert_image_side_identical(on, never, tag)
    assert_plain_records(on, pu, nu, sensors, tag)
    assert np.abs(on["records"][:, :3] - never["records"][:, :3]).max() > 1e-5       # the row times reached the solve
    BO.assert_records_identical(again["records"], on["records"], tag)
    assert_image_side_identical(off, never, tag)
    BO.assert_records_identical(off["records"], never["records"], tag)


@pytest.mark.parametrize("setting", ["robust", "cov", "gate", "seed", "camera", "several"])
def test_each_setting_with_the_rolling_shutter_on(pkg, ofk, setting):
    """Pair runs on two slices, gyro mode; `several` = camera, gates, seed and covariance at once.  (The zones belong to the streams.)"""
    from of_amd.pipeline import CameraModel, FlowPipeline
    prev, nxt, sensors = pair_batch(pkg, ofk)
    rs = R.rshutter(R.GYRO, -0.9, 0.0, H, omega_gain=1.0)
    cfg = {"robust": {}, "cov": COV, "gate": GATE, "seed": SEED, "camera": {}, "several": dict(COV, **GATE, **SEED)}[setting]
    cam = CameraModel(**PAIR_CAM).setting() if setting in ("camera", "several") else None
    pipe = FlowPipeline(W, H, B, pair_cfg(**cfg), streams=2)
    try:
        if setting == "robust":
            pipe.ctx.set_robust(**ROBUST)
        if cam is not None:
            pipe.ctx.set_camera(cam)
        pipe.upload(prev, nxt, sensors)
        off = pipe.run()
        pipe.ctx.set_rolling_shutter(as_struct(ofk, dict(rs, rows=0)))
        on = pipe.run()
        pu, nu = corrected_of_download(pipe.ctx, ofk, rs, on, sensors, setting, camera=cam)
        if cam is not None:                                      # both downloads are "what the solve stage saw"
            cp, cn = pipe.ctx.camera_download(B)
            assert np.array_equal(bits(cp), bits(pu)) and np.array_equal(bits(cn), bits(nu))
        if setting == "robust":
            wts, st = pipe.ctx.robust_download(B)
        if setting in ("cov", "several"):
            cov = pipe.covariances()
        if setting in ("gate", "several"):
            stats = pipe.track_gate_stats()
    finally:
        pipe.close()
    assert_image_side_identical(on, off, setting)                # a seeded LK predicts its seeds exactly as with the setting off
    assert np.abs(on["records"][:, :3] - off["records"][:, :3]).max() > 1e-5
    if setting != "robust":
        assert_plain_records(on, pu, nu, sensors, setting)
    if setting in ("gate", "several"):
        assert stats[:, 0].min() > 8, stats
    for b in range(B):
        n = int(on["counts"][b]); sr = sensors[b]
        ok = on["status"][b, :n] == 1
        new = nu[b, :n].astype(np.float64); old = pu[b, :n].astype(np.float64)
        if setting == "robust":
            x = (new - [sr[20], sr[21]]) * sr[19]; u = (new - old) * sr[19]
            ref = robust_reference(b, x, u, ok, sr, st[b])
            np.testing.assert_allclose(on["records"][b, 0:3], ref["v"], rtol=0, atol=1e-10, err_msg=str(b))
            np.testing.assert_allclose(wts[b, :n], ref["weights"], rtol=0, atol=1e-9, err_msg=str(b))
        if setting in ("cov", "several"):
            ref = cr.pair_record(cr.NODE, pu[b, :n], nu[b, :n], on["status"][b, :n], sr, COVD, on["records"][b])
            assert ref[13] == 0 and cov[b, 13] == 0
            for sl in (slice(0, 6), slice(6, 12), slice(16, 22)):
                assert np.abs(cov[b, sl] - ref[sl]).max() <= 1e-9 * np.abs(ref[sl]).max(), (b, sl)


# ---------------------------------------------------------------------------------------------------- streams


def run_stream(ofk, kind, frames, sensors, cfg, rshutter):
    """The device's steps: per step dict(rec, tracks, counts, nxt, keep, zones, ideal)."""
    from of_amd.pipeline import FlowStream, FusionConfig
    fusion = None if kind == "step" else FusionConfig(use_imu=False, redetect_replace=kind == "replace")
    fs = FlowStream(SW, SH, batch=NB, cfg=cfg, min_features=MIN_FEAT, mask_radius=RADIUS, fusion=fusion)
    try:
        if rshutter is not None:
            fs.ctx.set_rolling_shutter(rshutter)
        tracks, counts = fs.begin(frames[:, 0])
        steps = [dict(tracks=tracks, counts=counts)]
        for t in range(1, frames.shape[1]):
            out = fs.step(frames[:, t], sensors) if kind == "step" else fs.step_fused(frames[:, t], sensors)
            nxt, keep = fs.ctx.stream_last_points(cfg.max_corners)
            steps.append(dict(rec=out[0], tracks=out[-2], counts=out[-1], nxt=nxt, keep=keep, zones=fs.zones(),
                              ideal=fs.ideal_points() if rshutter is not None else None))
        return steps
    finally:
        fs.close()


@pytest.mark.parametrize("kind,mode", [("step", R.FLOW), ("fused", R.GYRO), ("replace", R.GYRO)])
def test_stream_steps_with_zones_and_the_rolling_shutter(pkg, ofk, sctx, kind, mode):
    frames, sensors, cfg = stream_setup(pkg, ofk, kind)
    rs = R.rshutter(mode, 0.9, 0.5, SH)
    m = as_struct(ofk, rs)
    on = run_stream(ofk, kind, frames, sensors, cfg, as_struct(ofk, dict(rs, rows=0)))
    off = run_stream(ofk, kind, frames, sensors, cfg, None)
    given = [dict() for _ in range(NB)]
    loops = [R.rs_loop(frames[b, 0], cfg, MIN_FEAT, RADIUS, rs, sensors[b], plain_solve if kind == "step" else feasibility_solve(sensors[b, 22:25], FEAS_T, 2),
                       given=given[b], zones={}, replace=kind == "replace") for b in range(NB)]
    for b in range(NB):
        assert np.array_equal(bits(on[0]["tracks"][b, :on[0]["counts"][b]]), bits(loops[b].tracks))
    same, solved, moved = True, 0, 0.0                           # the image side equals the setting-off run's until the keep flags part
    for t in range(1, NSTEPS + 1):
        s, s_off = on[t], off[t]
        for b in range(NB):
            tag = (kind, t, b)
            given[b]["pts"] = (s["ideal"][0][b], s["ideal"][1][b])     # the solver takes the device's corrected points: one ulp apart in gyro mode
            o = loops[b].step(frames[b, t], sensors[b])
            n = o["n_old"]
            assert n > 0, tag                                    # (a replacing re-detection leaves as few as two)
            assert np.array_equal(bits(s["nxt"][b, :n]), bits(o["new"])), tag
            pu, nu = s["ideal"][0][b, :n], s["ideal"][1][b, :n]
            sp, sn = sctx.rs_correct_points(m, o["old"], s["nxt"][b, :n], sensors=sensors[b:b + 1])
            assert np.array_equal(bits(pu), bits(sp)) and np.array_equal(bits(nu), bits(sn)), tag          # the composition
            assert same_points(pu, o["ideal"][0], ulp_of(mode)) and same_points(nu, o["ideal"][1], ulp_of(mode)), tag
            if o["keep"].any():
                moved = max(moved, float(np.abs(nu - s["nxt"][b, :n])[o["keep"]].max()))
            rec = s["rec"][b]
            assert rec[12] == n and rec[13] == o["n_tracked"] and rec[11] == o.get("used", o["n_tracked"]) and s["counts"][b] == len(o["tracks"]), (tag, rec[11:14])
            assert np.array_equal(s["keep"][b, :n] != 0, o["keep"]), tag
            assert np.array_equal(bits(s["tracks"][b, :s["counts"][b]]), bits(o["tracks"].astype(np.float32))), tag
            if o["solved"]:
                solved += 1
                np.testing.assert_allclose(rec[:3], o["v"], rtol=0, atol=1e-10, err_msg=str(tag))
                np.testing.assert_allclose(rec[8:11], o["v_uav"], rtol=0, atol=1e-10, err_msg=str(tag))
        if same:
            assert np.array_equal(bits(s["nxt"]), bits(s_off["nxt"])), (kind, t)            # same tracks in, same LK out
            same = np.array_equal(s["keep"], s_off["keep"])
            if same:
                assert np.array_equal(s["counts"], s_off["counts"]) and np.array_equal(bits(s["tracks"]), bits(s_off["tracks"])), (kind, t)
                for k in ("zones", "motion", "stats"):
                    assert np.array_equal(bits(s["zones"][k]), bits(s_off["zones"][k])), (kind, t, k)
                assert np.abs(s["rec"][:, :3] - s_off["rec"][:, :3]).max() > 1e-7        # and yet another solve
    print(f"{kind}: solved {solved}, largest correction {moved:.3f} px, image side equal to the setting off throughout: {same}")
    redetected = sum(1 for t in range(1, NSTEPS + 1) if (on[t - 1]["counts"] <= MIN_FEAT).any())
    assert solved >= NB * NSTEPS - 2 and moved > 0.003 and redetected > 0


def test_off_is_off(pkg, ofk):
    """A context that ran streams with the setting on (its buffers exist) and had it switched off returns, from the next begin on, the
    bits of a fresh context - for the plain and the fused step."""
    from of_amd.pipeline import FlowStream, FusionConfig
    for fused in (False, True):
        frames, sensors, cfg = stream_setup(pkg, ofk, "fused" if fused else "step")
        res = []
        for touch in (False, True):
            fs = FlowStream(SW, SH, batch=NB, cfg=cfg, min_features=MIN_FEAT, mask_radius=RADIUS, fusion=FusionConfig(use_imu=False) if fused else None)
            step = (lambda t: fs.step_fused(frames[:, t], sensors)) if fused else (lambda t: fs.step(frames[:, t], sensors))
            try:
                if touch:
                    fs.ctx.set_rolling_shutter(readout=0.9, mode="gyro")
                    fs.begin(frames[:, 0])
                    step(1); step(2)
                    fs.ideal_points()
                    fs.ctx.set_rolling_shutter(None)
                    assert fs.ctx.get_rolling_shutter().mode == ofk.RS_OFF
                    fs.ctx.zones_reset()
                fs.begin(frames[:, 0])
                res.append([tuple(step(t)) + tuple(fs.ctx.stream_last_points(cfg.max_corners)) + (fs.zones(),) for t in range(1, NSTEPS + 1)])
            finally:
                fs.close()
        for t, (x, y) in enumerate(zip(*res)):
            for i in range(len(x) - 1):
                assert np.array_equal(bits(x[i]), bits(y[i])), (fused, t, i)
            for k in ("zones", "motion", "stats"):
                assert np.array_equal(bits(x[-1][k]), bits(y[-1][k])), (fused, t, k)


# ---------------------------------------------------------------------------------------------------- the rendered scene
def test_rendered_scene_through_a_rolling_shutter_on_the_device(pkg, ofk):
    from of_amd.pipeline import FlowPipeline, PipelineConfig, RollingShutter
    fr0, sr, cfg, _ = R.scene(0.0)
    fr, sr, cfg, rs = R.scene()
    s = R.SCENE
    chain = BO.oracle_chain(fr["prev"], fr["next"], cfg, sr)
    pipe = FlowPipeline(s["w"], s["h"], 2, PipelineConfig(**{**cfg.__dict__, "rolling_shutter": RollingShutter(readout=s["readout"], mode="gyro", anchor=s["anchor"])}))
    try:
        pipe.upload(np.stack([fr["prev"], fr0["prev"]]), np.stack([fr["next"], fr0["next"]]), np.stack([sr, sr]))
        on = pipe.run()
        pu, nu = pipe.ideal_points()
        pipe.ctx.set_rolling_shutter(None)
        off = pipe.run()
    finally:
        pipe.close()
    n = int(on["counts"][0])
    assert n == len(chain["pts"])
    for k, r in (("prev_pts", "pts"), ("next_pts", "nxt"), ("status", "status"), ("err", "err")):
        assert np.array_equal(bits(on[k][0, :n]), bits(chain[r])), k
    ra, rb = R.correct_points(rs, chain["pts"], chain["nxt"], sensors=sr[None])
    assert same_points(pu[0, :n], ra, 1) and same_points(nu[0, :n], rb, 1)
    ok = chain["status"] == 1
    np.testing.assert_allclose(on["records"][0, :3], R.solve_points(pu[0, :n][ok], nu[0, :n][ok], sr), rtol=0, atol=1e-10)
    BO.assert_pair_matches(off, 0, chain, "the rolling-shutter frames, setting off")
    e_on, e_off, e_gs = R.rel_err(on["records"][0, :3]), R.rel_err(off["records"][0, :3]), R.rel_err(off["records"][1, :3])
    print("readout 0", e_gs, "gyro", e_on, "uncorrected", e_off)
    assert e_off >= 3.0 * e_gs and 4.0 * abs(e_on - e_gs) <= abs(e_off - e_on), (e_gs, e_on, e_off)
