"""GPU parity, whole resident pipeline (ofk_pairs_run): corners and LK bit-exact vs the oracle chain, recovered
velocity within 1e-9 relative of the lstsq oracle (north_star: 1e-4) and near the rendered truth."""
import numpy as np
import pytest

from oracle import image_oracle as io, estimation_oracle as eo

pytestmark = pytest.mark.gpu


def oracle_chain(prev, nxt, cfg, sensors_row, variant_sim=False):
    g0, g1 = io.gray_bgr8(prev), io.gray_bgr8(nxt)
    pts = io.good_features(g0, cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size)
    n, s, e = io.lk_pyr(g0, g1, pts, cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr)
    ok = s.ravel() == 1
    d, nrm, om = sensors_row[0], sensors_row[1:4], sensors_row[4:7]
    sc, cx, cy = sensors_row[19], sensors_row[20], sensors_row[21]
    new = n.reshape(-1, 2).astype(np.float64); old = pts.reshape(-1, 2).astype(np.float64)
    x = (new[ok] - [cx, cy]) * sc; u = (new[ok] - old[ok]) * sc
    if cfg.use_feasibility:
        r, _ = eo.r_tilde(x, u, nrm, sensors_row[22:25], d)
        x, u = x[r <= cfg.feas_T], u[r <= cfg.feas_T]
    v, R, rank, sv = eo.solve_lgs_node(x, u, d, nrm, om)
    v_uav = eo.post_solve(v, sensors_row[7:16].reshape(3, 3), om, sensors_row[16:19])
    return dict(pts=pts, nxt=n, status=s, err=e, v=v, R=R, rank=rank, s=sv, v_uav=v_uav, used=len(x))


@pytest.mark.parametrize("h,w,batch,preset", [(480, 640, 3, "evaluate"), (480, 640, 2, "node"), (1080, 1920, 2, "baseline")])
def test_pairs_pipeline_vs_oracle(pkg, ofk, h, w, batch, preset):
    from of_amd import synth
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    cfg = {"evaluate": PipelineConfig.evaluate_exp(), "node": PipelineConfig.node(), "baseline": PipelineConfig.baseline_1080p()}[preset]
    if preset != "baseline":
        cfg.quality = 0.1          # the reference's 0.7 leaves a handful of corners on this texture; keep the solve meaningful
    pairs = [synth.render_pair(h, w, 50 + b, v=(0.003 + 0.001 * b, -0.002, 0.0015), omega=(0.002, -0.001 * b, 0.004), d=1.0 + 0.5 * b)
             for b in range(batch)]
    prev = np.stack([p["prev"] for p in pairs]); nxt = np.stack([p["next"] for p in pairs])
    th = 0.1
    Rm = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    sensors = np.concatenate([ofk.make_sensors(1, d=p["d"], normal=p["n"], omega=p["omega"], rotation=Rm, scaling=p["scaling"],
                                               cx=p["cx"], cy=p["cy"]) for p in pairs])
    pipe = FlowPipeline(w, h, batch, cfg)
    pipe.upload(prev, nxt, sensors)
    out = pipe.run()
    for b in range(batch):
        ref = oracle_chain(prev[b], nxt[b], cfg, sensors[b])
        n = int(out["counts"][b])
        assert n == len(ref["pts"]) and n > 8
        assert np.array_equal(out["prev_pts"][b, :n], ref["pts"].reshape(-1, 2))
        assert np.array_equal(out["status"][b, :n], ref["status"].ravel())
        assert np.array_equal(out["next_pts"][b, :n].view(np.uint32), ref["nxt"].reshape(-1, 2).view(np.uint32))
        assert np.array_equal(out["err"][b, :n].view(np.uint32), ref["err"].ravel().view(np.uint32))
        rec = out["records"][b]
        np.testing.assert_allclose(rec[0:3], ref["v"], rtol=1e-9, atol=1e-13)
        np.testing.assert_allclose(rec[5:8], ref["s"], rtol=1e-9)
        np.testing.assert_allclose(rec[8:11], ref["v_uav"], rtol=1e-9, atol=1e-13)
        assert rec[4] == ref["rank"] and rec[11] == ref["used"] and rec[12] == n and rec[13] == int((ref["status"] == 1).sum())
        np.testing.assert_allclose(rec[3], ref["R"][0], rtol=1e-6, atol=1e-18)
        # and the estimate is physically right: within 2 % of the rendered per-frame velocity (6 % for the node preset)
        # measured: 0.4-0.7 % (evaluate, baseline presets), 3.0-4.3 % with the node preset's 100 block-12 corners on this render
        rel = np.linalg.norm(rec[0:3] - pairs[b]["v"]) / np.linalg.norm(pairs[b]["v"])
        assert rel < (0.06 if preset == "node" else 0.02), rel
    pipe.close()


def test_pairs_feasibility_filter_and_rerun_idempotent(pkg, ofk):
    from of_amd import synth
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    cfg = PipelineConfig(max_corners=200, quality=0.02, min_distance=8, block_size=7, use_feasibility=True, feas_T=-0.5)
    p = synth.render_pair(360, 480, 77, v=(0.004, 0.003, -0.001), omega=(0, 0, 0), d=1.0)
    sensors = ofk.make_sensors(1, d=1.0, normal=p["n"], omega=(0, 0, 0), scaling=p["scaling"], cx=p["cx"], cy=p["cy"], v_prior=p["v"])
    pipe = FlowPipeline(480, 360, 1, cfg)
    pipe.upload(p["prev"][None], p["next"][None], sensors)
    a = pipe.run(); b = pipe.run()
    for k in ("records", "prev_pts", "next_pts", "status", "err", "counts"):
        assert np.array_equal(a[k], b[k]), k                      # bitwise reproducible run to run
    ref = oracle_chain(p["prev"], p["next"], cfg, sensors[0])
    assert a["records"][0, 11] == ref["used"] and 3 <= ref["used"] <= a["records"][0, 13]
    np.testing.assert_allclose(a["records"][0, 0:3], ref["v"], rtol=1e-9, atol=1e-13)
    pipe.close()


@pytest.mark.parametrize("h,w,bs", [(257, 333, 7), (479, 641, 3), (250, 322, 5), (300, 404, 12), (240, 320, 9)])
def test_pairs_pipeline_odd_sizes_and_block_sizes(pkg, ofk, h, w, bs):
    """Widths that are not multiples of 4 take the byte-granular staging paths; block sizes 3/5/7/12 run the streaming
    response kernel, 9 the LDS-tile kernel.  All must agree with the oracle bit for bit."""
    from of_amd import synth
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    cfg = PipelineConfig(max_corners=120, quality=0.03, min_distance=7, block_size=bs, win=15, max_level=3)
    pairs = [synth.render_pair(h, w, 300 + b, v=(0.005, -0.004, 0.002), omega=(0.004, 0.002, -0.005), d=1.0) for b in range(2)]
    prev = np.stack([p["prev"] for p in pairs]); nxt = np.stack([p["next"] for p in pairs])
    sensors = np.concatenate([ofk.make_sensors(1, d=1.0, normal=p["n"], omega=p["omega"], scaling=p["scaling"], cx=p["cx"], cy=p["cy"]) for p in pairs])
    pipe = FlowPipeline(w, h, 2, cfg)
    pipe.upload(prev, nxt, sensors)
    out = pipe.run()
    for b in range(2):
        ref = oracle_chain(prev[b], nxt[b], cfg, sensors[b])
        n = int(out["counts"][b])
        assert n == len(ref["pts"]) and n > 8
        assert np.array_equal(out["prev_pts"][b, :n], ref["pts"].reshape(-1, 2))
        assert np.array_equal(out["status"][b, :n], ref["status"].ravel())
        assert np.array_equal(out["next_pts"][b, :n].view(np.uint32), ref["nxt"].reshape(-1, 2).view(np.uint32))
        np.testing.assert_allclose(out["records"][b, 0:3], ref["v"], rtol=1e-9, atol=1e-13)
    pipe.close()


def test_streams_do_not_change_results(pkg, ofk):
    """Cutting the batch into concurrent slices (HIP streams) is a scheduling choice only: bit-identical outputs."""
    from of_amd import synth
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    prev, nxt, base = synth.make_batch(5, 240, 320, seed=90, distinct=5)
    sensors = ofk.make_sensors(5, scaling=base[0]["scaling"], cx=base[0]["cx"], cy=base[0]["cy"])
    cfg = PipelineConfig(max_corners=80, quality=0.03, min_distance=6)
    outs = []
    for streams, overlap in ((1, False), (1, True), (2, True), (4, False), (8, True)):
        pipe = FlowPipeline(320, 240, 5, cfg, streams=streams)
        pipe.ctx.set_overlap(overlap)
        pipe.upload(prev, nxt, sensors)
        for _ in range(3):
            pipe.run_async()                                   # back to back: the auxiliary stream runs a call ahead
        outs.append(pipe.run())                                # 4th run: both pyramid sets reused under the same schedule
        pipe.close()
    for o in outs[1:]:
        assert np.array_equal(o["counts"], outs[0]["counts"])
        for b in range(5):
            n = int(o["counts"][b])
            for k in ("prev_pts", "next_pts", "status", "err"):
                assert np.array_equal(o[k][b, :n], outs[0][k][b, :n]), k
        assert np.array_equal(o["records"], outs[0]["records"])


def test_marks(pkg, ofk):
    """ofk_mark / ofk_mark_wait: waiting for step k's mark returns its complete records while step k+1 is queued behind."""
    from of_amd import synth
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    prev, nxt, base = synth.make_batch(3, 240, 320, seed=12, distinct=3)
    pipe = FlowPipeline(320, 240, 3, PipelineConfig(max_corners=64, quality=0.05))
    pipe.upload(prev, nxt, ofk.make_sensors(3, scaling=base[0]["scaling"], cx=base[0]["cx"], cy=base[0]["cy"]))
    ref = pipe.run()["records"]
    pipe.ctx.mark_wait(5)                                       # never marked: returns at once
    for k in range(4):
        pipe.run_async()
        pipe.ctx.mark(k % 2)
        if k:
            pipe.ctx.mark_wait((k - 1) % 2)
    pipe.ctx.mark_wait(1)
    assert np.array_equal(pipe.ctx.pairs_download(points=False)["records"], ref)
    with pytest.raises(ofk.OfkError):
        pipe.ctx.mark(8)
    pipe.close()


@pytest.mark.parametrize("streams", [2, 3])
def test_free_running_slices_export_and_join(pkg, ofk, streams):
    """With more than one slice stream the slices free-run over consecutive ofk_pairs_run calls; record export and marks run
    beside them on their own stream, and any other entry point joins them first.  None of that may change a single bit."""
    import ctypes
    from of_amd import synth
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    hip = ctypes.CDLL("libamdhip64.so")                        # the runtime libofk.so already loaded: plain device buffers, no torch
    B = 6
    nbytes = B * 8 * 4                                         # exported record: [v(3), R, used, s_min, rank, corners] as f32

    def dev_fill():
        assert hip.hipMemset(ctypes.c_void_p(ptr.value), 0xff, ctypes.c_size_t(2 * nbytes)) == 0

    def dev_read(slot):
        host = np.empty((B, 8), np.float32)
        assert hip.hipMemcpy(host.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr.value + slot * nbytes), ctypes.c_size_t(nbytes), 2) == 0
        return host
    prev, nxt, base = synth.make_batch(B, 240, 320, seed=31, distinct=B)
    s_a = ofk.make_sensors(B, scaling=base[0]["scaling"], cx=base[0]["cx"], cy=base[0]["cy"])
    s_b = ofk.make_sensors(B, scaling=base[0]["scaling"] * 1.25, cx=base[0]["cx"], cy=base[0]["cy"])
    cfg = PipelineConfig(max_corners=80, quality=0.03, min_distance=6)
    one = FlowPipeline(320, 240, B, cfg, streams=1)
    one.upload(prev, nxt, s_a)
    ref_a = one.run()
    one.ctx.pairs_set_sensors(s_b)
    ref_b = one.run()["records"]
    one.close()
    assert not np.array_equal(ref_a["records"], ref_b)

    pipe = FlowPipeline(320, 240, B, cfg, streams=streams)
    pipe.upload(prev, nxt, s_a)
    ptr = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(ptr), ctypes.c_size_t(2 * nbytes)) == 0
    dev_fill()
    want = ref_a["records"][:, [0, 1, 2, 3, 11, 7, 4, 12]].astype(np.float32)
    for k in range(5):                                         # export k overlaps run k+1; waiting on mark k-1 while k runs
        pipe.run_async()
        pipe.ctx.pairs_export_records_f32(ptr.value + (k % 2) * nbytes, B)
        pipe.ctx.mark(k % 2)
        if k:
            pipe.ctx.mark_wait((k - 1) % 2)
            assert np.array_equal(dev_read((k - 1) % 2).view(np.uint32), want.view(np.uint32))
    pipe.ctx.mark_wait(0)
    assert np.array_equal(dev_read(0).view(np.uint32), want.view(np.uint32))
    pipe.ctx.pairs_set_sensors(s_b)                            # joins the slices, then changes what the solve reads
    pipe.run_async()
    pipe.run_async()
    out = pipe.ctx.pairs_download()                            # joins again
    assert np.array_equal(out["records"], ref_b)
    assert np.array_equal(out["counts"], ref_a["counts"])
    for b in range(B):
        n = int(out["counts"][b])
        for key in ("prev_pts", "next_pts", "status", "err"):
            assert np.array_equal(out[key][b, :n], ref_a[key][b, :n]), key
    pipe.ctx.set_streams(1)                                    # joins; the next call runs on the context's stream alone
    pipe.ctx.pairs_set_sensors(s_a)
    assert np.array_equal(pipe.run()["records"], ref_a["records"])
    pipe.close()
    assert hip.hipFree(ptr) == 0


def test_profile_and_export(pkg, ofk):
    from of_amd import synth
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    p = synth.render_pair(240, 320, 5)
    pipe = FlowPipeline(320, 240, 1, PipelineConfig(max_corners=64, quality=0.05))
    pipe.upload(p["prev"][None], p["next"][None], ofk.make_sensors(1, scaling=p["scaling"], cx=p["cx"], cy=p["cy"]))
    pipe.ctx.profile_enable(0x7f)
    for _ in range(3):
        pipe.run_async()
    prof = pipe.ctx.profile_read()
    # 'nms' has no launches of its own: threshold + 3x3 NMS are fused into the response kernel ('eig'); 'gray' is timed
    # once per frame of the pair (the two conversions are separate launches on the auxiliary stream)
    assert all(prof[s][1] == (6 if s == "gray" else 3) and prof[s][0] > 0 for s in ofk.STAGES if s != "nms") and prof["nms"][1] == 0
    pipe.close()


@pytest.mark.parametrize("h,w,streams", [(1080, 1920, 1), (1080, 1920, 2), (480, 640, 1), (264, 2064, 1), (270, 480, 1)])
def test_resident_pyramids_after_a_pairs_run(pkg, ofk, h, w, streams):
    """The gray level and every pyramid level ofk_pairs_run leaves in HBM, byte for byte against cvtColor + pyrDown of the oracle:
    the three-levels-in-one-pass kernel (w % 16 == 0, h % 8 == 0; one, two and three strips; several chunks) and the per-level path
    (270 x 480), with one stream and with two free-running slices (double-buffered pyramid sets), twice in a row."""
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    rng = np.random.default_rng(h + w)
    batch = 4
    cfg = PipelineConfig.baseline_1080p()
    prev = rng.integers(0, 256, (batch, h, w, 3), dtype=np.uint8)
    nxt = rng.integers(0, 256, (batch, h, w, 3), dtype=np.uint8)
    prev[1, :, : w // 2] = 255; nxt[2, h // 3:] = 0                                    # saturated and black regions
    sensors = ofk.make_sensors(batch, d=1.0, normal=(0, 0, 1), omega=(0, 0, 0), scaling=1e-3, cx=w / 2, cy=h / 2)
    pipe = FlowPipeline(w, h, batch, cfg, streams=streams)
    pipe.upload(prev, nxt, sensors)
    for _ in range(2):
        pipe.run()
        for b in range(batch):
            for fs, frames in ((0, prev), (1, nxt)):
                ref = io.pyramid(io.gray_bgr8(frames[b]), cfg.win, cfg.max_level)
                got = pipe.ctx.resident_pyramid(fs, b, h, w, len(ref) - 1)
                for l, (g, r) in enumerate(zip(got, ref)):
                    assert np.array_equal(g, r), f"image {b} frame set {fs} level {l}: {np.argwhere(g != r)[:4]}"


@pytest.mark.parametrize("use_feas", [False, True])
def test_solve_kernels_agree_bit_for_bit(pkg, ofk, use_feas):
    """ofk_pairs_run solves with one WAVE per pair from 128 pairs on (k_pairs_solve: it fits beside the response kernel) and with a
    256-thread workgroup per pair below that (k_pairs_solve_wg).  The single wave forms its sums as the workgroup's four waves do -
    four virtual waves, the same shuffle butterfly, (s0 + s1) + (s2 + s3) - so the records of the same pairs are the same bits."""
    from of_amd import synth
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    h, w, D = 240, 320, 3
    pairs = [synth.render_pair(h, w, 20 + b, v=(0.004, -0.003 + 0.001 * b, 0.002), omega=(0.003, -0.002, 0.004)) for b in range(D)]
    cfg = PipelineConfig(max_corners=300, quality=0.01, min_distance=4, block_size=7, max_level=2, use_feasibility=use_feas, feas_T=0.5)
    outs = []
    for B in (D, 128 + D):
        prev = np.stack([pairs[b % D]["prev"] for b in range(B)]); nxt = np.stack([pairs[b % D]["next"] for b in range(B)])
        sensors = np.concatenate([ofk.make_sensors(1, d=pairs[b % D]["d"], normal=pairs[b % D]["n"], omega=pairs[b % D]["omega"], scaling=pairs[b % D]["scaling"],
                                                   cx=pairs[b % D]["cx"], cy=pairs[b % D]["cy"], v_prior=pairs[b % D]["v"]) for b in range(B)])
        pipe = FlowPipeline(w, h, B, cfg)
        pipe.upload(prev, nxt, sensors)
        out = pipe.run()
        rec = out["records"]
        # the stand-alone k_solve on x, u formed on the host from the same points (padded with invalid points) forms the same sums
        n = out["counts"]; S = int(n.max())
        nx = out["next_pts"][:, :S].astype(np.float64); pv = out["prev_pts"][:, :S].astype(np.float64)
        x = (nx - sensors[:, None, 20:22]) * sensors[:, 19, None, None]; u = (nx - pv) * sensors[:, 19, None, None]
        valid = (out["status"][:, :S] != 0) & (np.arange(S) < n[:, None])
        if use_feas:                                             # r_tilde with the prior velocity, as the pair kernels filter
            r, _ = pipe.ctx.feasibility(ofk.FEAS_RTILDE, x, u, sensors[:, 1:4], sensors[:, 22:25], dist=sensors[:, 0])
            valid &= r <= cfg.feas_T
        sol = pipe.ctx.velocity_solve(ofk.SOLVE_NODE, x, u, d=sensors[:, 0], nrm=sensors[:, 1:4], omega=sensors[:, 4:7],
                                      valid=valid.astype(np.uint8))
        assert np.array_equal(sol.view(np.uint64), rec[:, :8].view(np.uint64)), np.argwhere(sol != rec[:, :8])[:4]
        outs.append(rec)
        pipe.close()
    small, big = outs
    assert np.all(small[:, 11] > 100)                            # > 256 corners per pair: every virtual wave has points
    for b in range(128 + D):
        assert np.array_equal(big[b].view(np.uint64), small[b % D].view(np.uint64)), b
