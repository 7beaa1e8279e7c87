"""GPU: a stream's gyro bias (ofk_set_gyro_bias / ofk_gyro_bias_step) against tests/bias_reference.py.

(b^, P) of the device lie within TOL_BIAS of the restatement's, in the measure of bias_reference.rel_dev: TOL_BIAS is the tolerance
tests/test_bias_reference.py pins on the CPU (16 x the largest deviation of the sequential filter from the batch fusion).  delta, NIS
and R are held to REC_TOL = 1e-9 of their block's largest entry, tests/test_gpu_joint.py's bound with its argument.  The omega used is
the host's omega_raw - b^ bit for bit, and a stream run with the setting on equals, bit for bit in every output, the run with the
setting off whose sensors (and IMU messages) carry that difference: that is what shows that everything behind the apply kernel reads
the corrected omega.  The frames are tests/second_stage_runs.py's: 120 x 160, 2 streams, 64 corners, three steps."""
import numpy as np
import pytest

import bias_reference as br
import joint_reference as jr
import second_stage_runs as ssr
from joint_checks import REC_TOL
from point_stage_helpers import bits
from test_bias_reference import TOL_BIAS, PATTERNS, B0, SIGMA_GYRO

pytestmark = pytest.mark.gpu
SEEN = dict(dev=0.0)
SIGMA_FLOW_PX = 0.2


def assert_bias_close(rec, ref, tag):
    """A device record against the reference's: flag, counters, kept points and the omegas to the bit, (b^, P) within TOL_BIAS, the rest
    within REC_TOL of its block."""
    assert rec[18] == ref[18], (tag, "flag", rec[18], ref[18], rec, ref)
    assert np.array_equal(rec[[20, 21, 28]], ref[[20, 21, 28]]) and not rec[29:].any(), (tag, rec[[20, 21, 28]], ref[[20, 21, 28]])
    assert np.array_equal(bits(rec[9:15]), bits(ref[9:15])), (tag, "omega raw / used", rec[9:15], ref[9:15])
    dev = br.rel_dev(rec[0:3], jr.untri(rec[3:9]), ref[0:3], jr.untri(ref[3:9]))
    SEEN["dev"] = max(SEEN["dev"], dev)
    assert dev <= TOL_BIAS, (tag, dev, rec[0:9], ref[0:9])
    for lo, hi in ((15, 18), (19, 20), (22, 28)):
        scale = np.abs(ref[lo:hi]).max()
        assert np.abs(rec[lo:hi] - ref[lo:hi]).max() <= REC_TOL * scale, (tag, lo, rec[lo:hi], ref[lo:hi])


def batch3(n, **kw):
    sc = [jr.scene(n, 700 * n + b, **kw) for b in range(3)]
    return tuple(np.stack([s[k] for s in sc]) for k in range(7))


def setting_of(ofk, s):
    return ofk.gyro_bias_setting(True, s["sigma_flow"], s["sigma_gyro"], s["q"], s["p0"], s["b0"], s["nis_max"], s["update"])


# ---------------------------------------------------------------------------------------------------- the stage entry
@pytest.mark.parametrize("n", jr.COUNTS)
def test_stage_entry(gpu_ctx, ofk, n):
    x, u, d, nrm, om0, v, om = batch3(n)
    mask = np.ones((3, n), np.uint8)
    if n > 8:
        mask[:, 4::3] = 0
    for variant in (ofk.SOLVE_NODE, ofk.SOLVE_SIM):
        for name, p0 in PATTERNS.items():
            s = br.setting(sigma_flow=jr.SIGMA_FLOW, sigma_gyro=SIGMA_GYRO, q=1e-10, p0=p0, b0=B0)
            raw = np.where(s["p0"] > 0, om + jr.GYRO_ERROR, om + s["b0"])
            for valid in (None, mask):
                state = np.stack([br.initial_state(s)] * 3)
                for step in range(2):                            # the second step starts from the first one's state
                    out, new = gpu_ctx.gyro_bias_step(variant, x, u, d=d, nrm=nrm, omega=raw, state=state, valid=valid, gyro_bias=setting_of(ofk, s))
                    used = raw - state[:, 0:3]
                    assert np.array_equal(bits(new[:, 12:15]), bits(used)) and np.array_equal(bits(new[:, 9:12]), bits(raw))
                    plain = gpu_ctx.velocity_solve(variant, x, u, d=d, nrm=nrm, omega=used, valid=valid)
                    assert np.array_equal(bits(out), bits(plain))                     # the solve at the corrected omega, untouched
                    for b in range(3):
                        ref, j = br.step(s, state[b], variant, x[b], u[b], d[b], nrm[b], raw[b], valid=None if valid is None else valid[b],
                                         v_s=out[b, :3], rss_s=out[b, 3], rank=out[b, 4])
                        assert ref[18] == (4 if name == "held" else 0), (n, name, ref[18])
                        assert_bias_close(new[b], ref, f"n {n} variant {variant} {name} valid {valid is not None} step {step} problem {b}")
                    if name == "held":
                        assert np.array_equal(bits(new[:, 0:9]), bits(state[:, 0:9]))
                    if name == "mixed":
                        assert np.array_equal(new[:, 0], state[:, 0]) and not new[:, 3:6].any()
                    state = new
    print(f"n {n}: largest deviation of (b^, P) so far {SEEN['dev']:.3e} (TOL_BIAS {TOL_BIAS:.2e})")


def test_stage_entry_with_the_robust_setting(gpu_ctx, ofk):
    n = 257
    x, u, d, nrm, om0, v, om = batch3(n, outliers=True)
    rob = ofk.robust_setting("tukey", hypotheses=32, seed=77)
    s = br.setting(sigma_flow=jr.SIGMA_FLOW, sigma_gyro=SIGMA_GYRO, q=1e-10, p0=1e-2, b0=B0)
    state = np.stack([br.initial_state(s)] * 3)
    for variant in (ofk.SOLVE_NODE, ofk.SOLVE_SIM):
        out, new = gpu_ctx.gyro_bias_step(variant, x, u, d=d, nrm=nrm, omega=om0, state=state, robust=rob, gyro_bias=setting_of(ofk, s))
        out_r, w, st = gpu_ctx.velocity_solve_robust(variant, x, u, d=d, nrm=nrm, omega=om0 - state[:, 0:3], robust=rob)
        assert np.array_equal(bits(out), bits(out_r)) and np.any((w > 0) & (w < 1))
        for b in range(3):
            ref, j = br.step(s, state[b], variant, x[b], u[b], d[b], nrm[b], om0[b], w=w[b], v_s=out[b, :3], rss_s=out[b, 3], rank=out[b, 4])
            assert ref[18] == 0 and new[b, 28] == np.count_nonzero(w[b] > 0)
            assert_bias_close(new[b], ref, f"robust variant {variant} problem {b}")


def test_stage_entry_flags(gpu_ctx, ofk):
    x, u, d, nrm, om0, v, om = batch3(65)
    s = br.setting(sigma_flow=jr.SIGMA_FLOW, sigma_gyro=SIGMA_GYRO, q=1e-8, p0=(1e-2, 0.0, 1e-2), b0=B0)
    state = np.stack([br.initial_state(s)] * 3)
    predicted = state[:, 3:9] + np.array([1e-8, 0, 0, 0, 0, 1e-8])
    good, gnew = gpu_ctx.gyro_bias_step(ofk.SOLVE_NODE, x, u, d=d, nrm=nrm, omega=om0, state=state, gyro_bias=setting_of(ofk, s))
    assert np.all(gnew[:, 18] == 0) and np.all(gnew[:, 20] == 1) and np.all(gnew[:, 21] == 1)
    # flag 1: a NaN range among finite problems, which keep their bits
    dd = d.copy(); dd[1] = np.nan
    out, new = gpu_ctx.gyro_bias_step(ofk.SOLVE_NODE, x, u, d=dd, nrm=nrm, omega=om0, state=state, gyro_bias=setting_of(ofk, s))
    assert new[1, 18] == 1 and np.array_equal(new[1, 0:3], B0) and np.array_equal(new[1, 3:9], predicted[1]) and new[1, 20] == 0 and new[1, 21] == 1
    assert not new[1, 15:18].any() and new[1, 19] == 0 and not new[1, 22:28].any()
    for b in (0, 2):
        assert np.array_equal(bits(new[b]), bits(gnew[b])) and np.array_equal(bits(out[b]), bits(good[b]))
    # flag 3: a gate the innovation does not pass; NIS and R are reported, the state only predicts
    gate = dict(s, nis_max=1e-3)
    out, new = gpu_ctx.gyro_bias_step(ofk.SOLVE_NODE, x, u, d=d, nrm=nrm, omega=om0, state=state, gyro_bias=setting_of(ofk, gate))
    assert np.array_equal(bits(out), bits(good))
    for b in range(3):
        ref, j = br.step(gate, state[b], jr.NODE, x[b], u[b], d[b], nrm[b], om0[b], v_s=out[b, :3], rss_s=out[b, 3], rank=out[b, 4])
        assert ref[18] == 3 and np.array_equal(new[b, 0:3], B0) and np.array_equal(new[b, 3:9], predicted[b]) and new[b, 20] == 0
        assert_bias_close(new[b], ref, f"gated problem {b}")
    # update off: apply only, the state stays
    out, new = gpu_ctx.gyro_bias_step(ofk.SOLVE_NODE, x, u, d=d, nrm=nrm, omega=om0, state=state, gyro_bias=setting_of(ofk, dict(s, update=False)))
    assert np.array_equal(bits(out), bits(good)) and np.all(new[:, 18] == 4) and np.array_equal(bits(new[:, 0:9]), bits(state[:, 0:9]))
    assert np.array_equal(bits(new[:, 12:15]), bits(om0 - B0)) and np.all(new[:, 21] == 1) and not new[:, 22:].any()


# ---------------------------------------------------------------------------------------------------- stream runs
def bias_keywords(**over):
    return dict(dict(sigma_flow=SIGMA_FLOW_PX, sigma_gyro=SIGMA_GYRO, q=1e-10, p0=(5e-3, 5e-3, 5e-3), b0=(2e-4, -1e-4, 1e-4), nis_max=0.0, update=True), **over)


def run(ofk, fusion_name, bias=None, corrections=None, robust=None, extra=None, reset=None, B=2, steps_n=3, drop=None, nan_gyro=None,
        blank=None, fusion=None):
    """B streams (the two clips in turn) x steps_n steps.  bias: gyro_bias_setting's keywords (run A) or None (run B); corrections: per
    step the [B, 3] that run B takes off the gyro on the host (sensors and IMU messages); extra: further PipelineConfig fields; reset: a
    state for gyro_bias_reset behind begin.  drop / nan_gyro: the step (1 ..) at which stream 1's range / second gyro axis (sensors and
    IMU messages) is NaN (stream 0's where there is one stream).  blank: a stream whose first frame is a uniform 128.  fusion: a FusionConfig in place of fusion_name's.
    Returns per step what the device reported."""
    from of_amd.pipeline import FlowStream
    from stream_oracle import imu_messages
    frames, info = ssr.stream_frames()
    frames = frames[np.arange(B) % 2]
    if blank is not None:
        frames = frames.copy(); frames[blank, 0] = 128
    cfg = ssr.pipeline_config(**dict(dict(robust=robust, robust_hypotheses=16, robust_iters=3, robust_seed=5) if robust else {}, **(extra or {})))
    fusion = ssr.make_fusion(fusion_name) if fusion is None else fusion
    use_imu = fusion is not None and fusion.use_imu
    sensors = ssr.stream_sensors(ofk, info)[np.arange(B) % 2]
    fs = FlowStream(ssr.W, ssr.H, batch=B, cfg=cfg, min_features=10, mask_radius=8, fusion=fusion)
    steps = []
    try:
        if bias is not None:
            fs.ctx.set_gyro_bias(**bias)
        tracks, counts = fs.begin(frames[:, 0])
        if reset is not None:
            fs.ctx.gyro_bias_reset(reset)
        rng = np.random.default_rng(31)
        for t in range(1, steps_n + 1):
            corr = np.zeros((B, 3)) if corrections is None else corrections[t - 1]
            given = sensors.copy()
            if drop == t:
                given[min(B, 2) - 1, 0] = np.nan
            if nan_gyro == t:
                given[min(B, 2) - 1, 5] = np.nan
            sr = given.copy()
            sr[:, 4:7] = given[:, 4:7] - corr
            imu = raw = None
            if use_imu:
                msgs = np.stack([imu_messages(rng, 0.1 * t + 10 * s, 3, rate=np.asarray(info["omega"]) + ssr.GYRO_OFF) for s in range(min(B, 2))])
                msgs = msgs[np.arange(B) % 2]                    # past two streams the clips' messages in turn, as the frames
                if nan_gyro == t:
                    msgs[min(B, 2) - 1, :, 7] = np.nan
                raw = msgs[:, -1, 6:9].copy()
                msgs[:, :, 6:9] = msgs[:, :, 6:9] - corr[:, None, :]
                fs.push_imu(msgs)
                imu = fs.ctx.imu_state(B)[0]
            old_tracks, old_counts = tracks.copy(), counts.copy()
            if fusion is None:
                rec, tracks, counts = fs.step(frames[:, t], sr)
                fused = x = P = None
            else:
                rec, fused, tracks, counts = fs.step_fused(frames[:, t], sr)
                x, P = fs.ctx.filter_state(B) if fusion.filter else (None, None)
            nxt, keep = fs.ctx.stream_last_points(ssr.CORNERS)
            imu_after = fs.ctx.imu_state(B)[0] if use_imu else None
            steps.append(dict(rec=rec, fused=fused, old=old_tracks, n=old_counts, nxt=nxt, keep=keep, imu=imu, x=x, P=P, imu_after=imu_after,
                              sr=sr, tracks=tracks.copy(), counts=counts.copy(), raw=raw if use_imu else given[:, 4:7].copy(),
                              bias=fs.gyro_bias() if bias is not None else None,
                              weights=fs.ctx.robust_download(B)[0] if robust else None))
    finally:
        fs.close()
    return steps, fusion


def assert_twin(a_steps, b_steps, use_imu, tag, counted=False):
    """Every output of run A equals run B's bit for bit; the IMU state but for its omega, which A holds raw and B corrected.  counted:
    the point arrays are compared up to each stream's count (a stream without tracks leaves the rows behind its count as they were)."""
    rows = {"tracks": "counts", "nxt": "n", "keep": "n"}
    for t, (a, b) in enumerate(zip(a_steps, b_steps)):
        for k in ("rec", "fused", "x", "P", "tracks", "counts", "nxt", "keep"):
            if a[k] is not None and counted and k in rows:
                assert np.array_equal(a[rows[k]], b[rows[k]]), (tag, t, rows[k], a[rows[k]], b[rows[k]])
                for s, n in enumerate(a[rows[k]]):
                    assert np.array_equal(bits(a[k][s, :n]), bits(b[k][s, :n])), (tag, t, k, s, a[k][s, :n], b[k][s, :n])
            elif a[k] is not None:
                assert np.array_equal(bits(a[k]), bits(b[k])), (tag, t, k, a[k], b[k])
        if use_imu:
            rest = np.r_[0:18, 21:24]
            assert np.array_equal(bits(a["imu_after"][:, rest]), bits(b["imu_after"][:, rest])), (tag, t, "IMU state")
            assert np.array_equal(bits(a["imu_after"][:, 18:21]), bits(a["raw"])), (tag, t, "the IMU state's omega is the raw one again")


def twin(ofk, fusion_name, bias, robust=None, extra=None, reference=True, reset=None, **how):
    """how: run's further keywords (B, steps_n, drop, nan_gyro, blank, fusion), the same in both runs."""
    counted = how.get("blank") is not None
    a, fusion = run(ofk, fusion_name, bias=bias, robust=robust, extra=extra, reset=reset, **how)
    B = how.get("B", 2)
    use_imu = fusion is not None and fusion.use_imu
    s = br.setting(**{k: v for k, v in bias.items()})
    start = np.stack([br.initial_state(s)] * B)
    if reset is not None:
        start[:, 0:9] = reset
    before = [start[:, 0:3]] + [st["bias"][:, 0:3] for st in a[:-1]]
    corrections = [np.array(b, np.float64) for b in before]
    for t, st in enumerate(a):                                   # the omega used is the host's difference, to the bit
        assert np.array_equal(bits(st["bias"][:, 9:12]), bits(st["raw"])), (fusion_name, t)
        assert np.array_equal(bits(st["bias"][:, 12:15]), bits(st["raw"] - corrections[t])), (fusion_name, t)
    b, _ = run(ofk, fusion_name, bias=None, corrections=corrections, robust=robust, extra=extra, **how)
    assert_twin(a, b, use_imu, (fusion_name, robust, extra), counted)
    if reference:
        state = start
        for t, st in enumerate(a):
            for k in range(B):
                n = int(st["n"][k])
                used = st["raw"][k] - state[k, 0:3]
                nrm = st["imu"][k, 15:18] if use_imu else None
                keepf = st["keep"][k, :n].astype(bool) if fusion is not None else None
                w = None if st["weights"] is None else st["weights"][k, :n]
                rec = st["rec"][k]
                j = jr.pair_joint(jr.NODE, st["old"][k, :n], st["nxt"][k, :n], st["keep"][k, :n], st["sr"][k], s["sigma_flow"],
                                  tuple(np.where(s["p0"] > 0, np.inf, 0.0)), rec, w=w, keep=keepf, nrm=nrm, omega=used,
                                  solved=fusion is None or rec[15] != 0)
                ref = br.filter_step(s, br.apply(state[k], st["raw"][k]), j)
                assert_bias_close(st["bias"][k], ref, f"{fusion_name} robust {robust} step {t} stream {k}")
            state = st["bias"]
    return a, b


@pytest.mark.parametrize("robust", (None, "tukey"))
@pytest.mark.parametrize("fusion_name", ssr.FUSIONS)
def test_twin_run(ofk, fusion_name, robust):
    a, b = twin(ofk, fusion_name, bias_keywords(), robust=robust)
    flags = np.stack([st["bias"][:, 18] for st in a])
    assert np.all(flags == 0), flags                             # every step updated: the bias moved and the twin still holds
    assert np.all(a[-1]["bias"][:, 20] == 3) and np.all(a[-1]["bias"][:, 21] == 3)
    assert not np.array_equal(a[0]["bias"][:, 0:3], a[-1]["bias"][:, 0:3])
    print(f"{fusion_name} robust {robust}: largest deviation of (b^, P) so far {SEEN['dev']:.3e}; b^ after three steps {a[-1]['bias'][:, 0:3]}")


def settings_that_read_omega():
    from of_amd.pipeline import RollingShutter
    return {"seed": dict(lk_seed="model", seed_gain=1.0), "rolling shutter": dict(rolling_shutter=RollingShutter(readout=0.5, mode="gyro")),
            "finite motion": dict(finite_motion=True), "joint": dict(joint=True, joint_sigma_flow_px=0.2, omega_prior=1e-3),
            "epipolar": dict(epipolar=True)}


@pytest.mark.parametrize("name", ("seed", "rolling shutter", "finite motion", "joint", "epipolar"))
def test_twin_run_beside_the_settings_that_read_omega(ofk, name):
    # the bias is large against the setting's own effect, so a reader of the raw omega would show; the reference's filter step is fed
    # with the image's points and the solve's own v, which only the seed leaves in place
    twin(ofk, "plain", bias_keywords(b0=(2e-3, -1e-3, 1e-3)), extra=settings_that_read_omega()[name], reference=name == "seed")


# ---------------------------------------------------------------------------------------------------- off-equivalence
@pytest.mark.parametrize("fusion_name", ssr.FUSIONS)
def test_zero_bias_held_is_the_setting_off(ofk, fusion_name):
    a, fusion = run(ofk, fusion_name, bias=bias_keywords(b0=0.0, p0=0.0))
    b, _ = run(ofk, fusion_name)
    use_imu = fusion is not None and fusion.use_imu
    assert_twin(a, b, use_imu, fusion_name)
    if use_imu:
        for sa, sb in zip(a, b):
            assert np.array_equal(bits(sa["imu_after"]), bits(sb["imu_after"]))
    assert np.all(a[-1]["bias"][:, 18] == 4) and not a[-1]["bias"][:, 0:9].any() and np.all(a[-1]["bias"][:, 21] == 3)


@pytest.mark.parametrize("fusion_name", ("plain", "node"))
def test_update_off_applies_and_never_changes(ofk, fusion_name):
    kw = bias_keywords(b0=(1e-3, -1e-3, 5e-4), update=False)
    a, b = twin(ofk, fusion_name, kw, reference=False)
    start = br.initial_state(br.setting(**kw))
    for t, st in enumerate(a):
        assert np.all(st["bias"][:, 18] == 4) and np.array_equal(bits(st["bias"][:, 0:9]), bits(np.stack([start[0:9]] * 2)))
        assert np.all(st["bias"][:, 20] == 0) and np.all(st["bias"][:, 21] == t + 1)


# ---------------------------------------------------------------------------------------------------- lifecycle
def test_begin_resets_and_reset_loads(ofk):
    from of_amd.pipeline import FlowStream
    frames, info = ssr.stream_frames()
    sensors = ssr.stream_sensors(ofk, info)
    kw = bias_keywords()
    start = br.initial_state(br.setting(**kw))
    fs = FlowStream(ssr.W, ssr.H, batch=2, cfg=ssr.pipeline_config(gyro_bias=ofk.gyro_bias_setting(**kw)), min_features=10, mask_radius=8)
    try:
        with pytest.raises(ofk.OfkError):                        # no step yet
            fs.gyro_bias()
        fs.begin(frames[:, 0])
        with pytest.raises(ofk.OfkError):                        # begun, still no step
            fs.gyro_bias()
        fs.step(frames[:, 1], sensors)
        first = fs.gyro_bias()
        assert np.all(first[:, 18] == 0) and np.all(first[:, 21] == 1) and np.array_equal(bits(first[:, 12:15]), bits(sensors[:, 4:7] - start[0:3]))
        fs.step(frames[:, 2], sensors)
        assert np.all(fs.gyro_bias()[:, 21] == 2)
        fs.begin(frames[:, 0])                                   # the state is the setting's again
        with pytest.raises(ofk.OfkError):
            fs.gyro_bias()
        fs.step(frames[:, 1], sensors)
        assert np.array_equal(bits(fs.gyro_bias()), bits(first))
        hot = np.stack([np.r_[first[0, 0:9]], np.r_[1e-3, 2e-3, -1e-3, 1e-6, 0, 0, 2e-6, 0, 3e-6]])
        fs.begin(frames[:, 0])
        fs.ctx.gyro_bias_reset(hot)
        fs.step(frames[:, 1], sensors)
        rec = fs.gyro_bias()
        assert np.array_equal(bits(rec[:, 12:15]), bits(sensors[:, 4:7] - hot[:, 0:3])) and np.all(rec[:, 21] == 1) and np.all(rec[:, 20] == 1) and np.all(rec[:, 18] == 0)
        fs.ctx.set_gyro_bias(**kw)                               # setting it again is the setting's start as well
        fs.step(frames[:, 2], sensors)
        assert np.array_equal(bits(fs.gyro_bias()[:, 12:15]), bits(sensors[:, 4:7] - start[0:3]))
        fs.ctx.gyro_bias_reset(hot[:1])                          # one stream of the two
        fs.step(frames[:, 3], sensors)
        assert np.array_equal(bits(fs.gyro_bias()[0, 12:15]), bits(sensors[0, 4:7] - hot[0, 0:3]))
    finally:
        fs.close()


def test_what_is_not_the_sensor_model_is_refused_while_updating(ofk):
    from of_amd.pipeline import FlowStream, FusionConfig
    frames, info = ssr.stream_frames()
    sensors = ssr.stream_sensors(ofk, info)
    cases = {"OFK_FLOW_ROTATIONAL": (ssr.pipeline_config(), FusionConfig(use_imu=False, flow=ofk.FLOW_ROTATIONAL)),
             "OFK_KEEP_LEGACY": (ssr.pipeline_config(), FusionConfig(use_imu=False, keep=ofk.KEEP_LEGACY)),
             "OFK_SOLVE_OFMODULE": (ssr.pipeline_config(solve_variant=ofk.SOLVE_OFMODULE), FusionConfig(use_imu=False, keep=ofk.KEEP_LEGACY))}
    for name, (cfg, fusion) in cases.items():
        for update in (True, False):
            fs = FlowStream(ssr.W, ssr.H, batch=2, cfg=cfg, min_features=10, mask_radius=8, fusion=fusion)
            try:
                fs.ctx.set_gyro_bias(**bias_keywords(update=update))
                fs.begin(frames[:, 0])
                if update:
                    with pytest.raises(ofk.OfkError) as e:
                        fs.step_fused(frames[:, 1], sensors)
                    assert e.value.code == ofk.E_INVALID and name in str(e.value) and "not the sensor model" in str(e.value), str(e.value)
                else:
                    fs.step_fused(frames[:, 1], sensors)
                    assert np.all(fs.gyro_bias()[:, 18] == 4)
            finally:
                fs.close()


def test_flow_pipeline_ignores_the_setting(ofk):
    from of_amd.pipeline import FlowPipeline
    prev, nxt, base = ssr.pair_frames(2)
    sensors = ssr.pair_sensors(ofk, 2, base)
    outs = []
    for on in (False, True):
        pipe = FlowPipeline(ssr.W, ssr.H, 2, ssr.pipeline_config(gyro_bias=True if on else None))
        try:
            if on:
                pipe.ctx.set_gyro_bias(**bias_keywords(b0=(1e-3, -1e-3, 5e-4)))              # even set on the context itself
            pipe.upload(prev, nxt, sensors)
            outs.append(pipe.run())
            if on:
                with pytest.raises(ofk.OfkError):                # no step: nothing to download
                    pipe.ctx.gyro_bias_download(2)
        finally:
            pipe.close()
    assert len(outs[0]) == len(outs[1]) and len(outs[0]) >= 1
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(bits(np.asarray(a)), bits(np.asarray(b)))
