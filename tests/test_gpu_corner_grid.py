"""The corner grid on the device (include/ofk.h: ofk_corner_grid) against its numpy restatement (tests/corner_grid_reference.py):
the two stage entries on every case of tests/corner_grid_cases.py bit for bit with equal statistics, the context setting, off and
non-binding settings against the plain entries, the refusals, and the resident chains (FlowPipeline.run, FlowStream in step,
step_fused and replace mode) with a binding grid against the oracle chain fed with the reference's corners."""
import numpy as np
import pytest

from oracle import image_oracle as io, estimation_oracle as eo
import corner_grid_cases as K
import corner_grid_reference as R
from batch_oracle import assert_pair_matches, grid_chain  # noqa: E402  (tests/batch_oracle.py)
from stream_oracle import NodeLoop, disc_mask, track  # noqa: E402  (tests/stream_oracle.py)

pytestmark = pytest.mark.gpu

H, W = 240, 320


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_matches(pts, counts, stats, refs, tag):
    for b, (want, st, _) in enumerate(refs):
        n = int(counts[b])
        assert n == len(want) and tuple(int(v) for v in stats[b]) == st, (tag, b, n, len(want), stats[b], st)
        assert np.array_equal(bits(pts[b, :n]), bits(want)), (tag, b)


@pytest.mark.parametrize("case", K.CASES, ids=[c["id"] for c in K.CASES])
def test_stage_entries_bit_for_bit(pkg, ofk, gpu_ctx, case):
    gray = K.images(case); B = len(gray)
    refs = K.reference(case)
    grid = ofk.corner_grid_setting(*case["grid"])
    args = (case["max_corners"], case["quality"], case["min_distance"])
    mask = None if case["mask"] is None else np.repeat(case["mask"], B, 0)[:B]
    for rerun in range(2):                                       # a second launch on the same buffers gives the same bits
        pts, counts = gpu_ctx.good_features(gray, *args, case["block"], mask=mask, grid=grid, occupied=case["occ"])
        assert_matches(pts, counts, gpu_ctx.corner_grid_stats(B), refs, (case["id"], "good_features_grid", rerun))
    eig = np.stack([K.eig_of(case["scene"], case["block"])] * B)
    pts2, counts2 = gpu_ctx.select_corners(eig, *args, mask=mask, grid=grid, occupied=case["occ"])
    assert_matches(pts2, counts2, gpu_ctx.corner_grid_stats(B), refs, (case["id"], "select_corners_grid"))
    assert gpu_ctx.get_corner_grid().cell == 0                   # the stage entries took their own setting: the context's stays off
    if case["occ"] is None:                                      # the context setting through the plain entry is the same call
        gpu_ctx.set_corner_grid(grid)
        try:
            pts3, counts3 = gpu_ctx.good_features(gray, *args, case["block"], mask=mask)
            assert np.array_equal(counts3, counts) and np.array_equal(bits(pts3), bits(pts)), case["id"]
            assert np.array_equal(gpu_ctx.corner_grid_stats(B), [r[1] for r in refs])
            pts4, counts4 = gpu_ctx.select_corners(eig, *args, mask=mask)
            assert np.array_equal(counts4, counts) and np.array_equal(bits(pts4), bits(pts)), case["id"]
        finally:
            gpu_ctx.set_corner_grid(None)
    if "plain" in case["designated"]:                            # a cap that cannot bind: the plain entry's output
        pp, pc = gpu_ctx.good_features(gray, *args, case["block"], mask=mask)
        assert np.array_equal(pc, counts) and np.array_equal(bits(pp), bits(pts)), case["id"]


@pytest.mark.parametrize("case", K.PLATEAU_CASES, ids=[c["id"] for c in K.PLATEAU_CASES])
def test_equal_values_and_plateaus(pkg, ofk, gpu_ctx, case):
    e = K.plateau_map()
    ref = K.plateau_reference(case)
    grid = ofk.corner_grid_setting(*case["grid"])
    eig = np.stack([e, e])
    for rerun in range(2):
        pts, counts = gpu_ctx.select_corners(eig, case["max_corners"], case["quality"], case["min_distance"], grid=grid)
        assert_matches(pts, counts, gpu_ctx.corner_grid_stats(2), [ref, ref], (case["id"], rerun))


def test_off_is_the_plain_entry(pkg, ofk, gpu_ctx):
    gray = K.scene("a")[None]
    for md in (0, 3):
        want, wc = gpu_ctx.good_features(gray, 64, 0.01, md, 3)
        ref = io.good_features(gray[0], 64, 0.01, md, 3).reshape(-1, 2)
        assert wc[0] == len(ref) and np.array_equal(bits(want[0, :wc[0]]), bits(ref))
        for grid in (ofk.CornerGrid(0, 0, 0), ofk.CornerGrid(0, -7, -7), ofk.corner_grid_setting(40, 64, 0), ofk.corner_grid_setting(40, 1 << 30, 0)):
            got, gc = gpu_ctx.good_features(gray, 64, 0.01, md, 3, grid=grid)
            assert np.array_equal(gc, wc) and np.array_equal(bits(got), bits(want)), (md, grid.cell, grid.cap)
        gpu_ctx.set_corner_grid(cell=40, cap=1)
        gpu_ctx.set_corner_grid(None)
        got, gc = gpu_ctx.good_features(gray, 64, 0.01, md, 3)
        assert np.array_equal(gc, wc) and np.array_equal(bits(got), bits(want))


def test_refusals(pkg, ofk):
    ctx = ofk.Context(0, 640, 480, 2, 64, 2)
    try:
        gray = K.scene("a")[None]
        with pytest.raises(ofk.OfkError, match="no selection with a corner grid"):
            ctx.corner_grid_stats(1)
        want, wc = ctx.good_features(gray, 64, 0.01, 3, 3)
        ctx.set_corner_grid(cell=40, cap=2)
        for bad in (ofk.CornerGrid(-1, 1, 0), ofk.CornerGrid(8, 0, 0), ofk.CornerGrid(8, -1, 0), ofk.CornerGrid(8, 1, -1)):
            with pytest.raises(ofk.OfkError) as ei:
                ctx.set_corner_grid(bad)
            assert ei.value.code == -1
            g = ctx.get_corner_grid()
            assert (g.cell, g.cap, g.max_rank) == (40, 2, 0)     # the setting stays
            with pytest.raises(ofk.OfkError) as ei:
                ctx.good_features(gray, 64, 0.01, 3, 3, grid=bad)
            assert ei.value.code == -1
            with pytest.raises(ofk.OfkError) as ei:
                ctx.select_corners(K.eig_of("a", 3)[None], 64, 0.01, 3, grid=bad)
            assert ei.value.code == -1
        ctx.set_corner_grid(None)
        assert -(-320 // 7) * -(-240 // 7) <= ofk.GRID_MAX_CELLS < -(-320 // 6) * -(-240 // 6)
        ctx.good_features(gray, 64, 0.01, 3, 3, grid=ofk.corner_grid_setting(7, 1))
        with pytest.raises(ofk.OfkError, match="OFK_GRID_MAX_CELLS"):
            ctx.good_features(gray, 64, 0.01, 3, 3, grid=ofk.corner_grid_setting(6, 1))
        ctx.set_corner_grid(cell=6, cap=1)                       # the frame is not known to the setter: the selecting call refuses
        with pytest.raises(ofk.OfkError, match="OFK_GRID_MAX_CELLS"):
            ctx.good_features(gray, 64, 0.01, 3, 3)
        ctx.set_corner_grid(None)
        occ = (np.zeros((1, 65, 2), np.float32), np.zeros(1, np.int32))
        with pytest.raises(ofk.OfkError, match="occ_stride"):    # an occupancy row longer than the context's max_pts
            ctx.good_features(gray, 64, 0.01, 3, 3, grid=ofk.corner_grid_setting(40, 1), occupied=occ)
        got, gc = ctx.good_features(gray, 64, 0.01, 3, 3)        # nothing was queued or left behind
        assert np.array_equal(gc, wc) and np.array_equal(bits(got), bits(want))
    finally:
        ctx.close()


CORNERS = dict(max_corners=60, quality=0.01, min_distance=5, block_size=5)
LK = dict(win=15, max_level=2, max_count=20, eps=0.03, min_eig_thr=1e-4)
MOTION = dict(v=(0.003, -0.002, 0.001), omega=(0.03, -0.02, 0.1))
STREAM_MOTION = dict(v=(0.003, -0.002, 0.001), omega=(0.015, -0.01, 0.05), d=1.0)


@pytest.mark.parametrize("slices", [1, 2])
def test_pairs_run_with_a_binding_grid(pkg, ofk, slices):
    from of_amd import synth
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    B, grid = 3, (40, 1, 0)
    cfg = PipelineConfig(grid_cell=grid[0], grid_cap=grid[1], grid_max_rank=grid[2], **CORNERS, **LK)
    pairs = [synth.render_pair(H, W, sd, margin=64, **MOTION) for sd in (5, 6, 7)]
    p = pairs[0]
    sensors = ofk.make_sensors(B, d=p["d"], normal=p["n"], omega=p["omega"], scaling=p["scaling"], cx=p["cx"], cy=p["cy"])
    refs = [grid_chain(q["prev"], q["next"], cfg, sensors[0], grid) for q in pairs]
    assert all(len(r["pts"]) >= 20 and not np.array_equal(r["pts"], r["plain"]) for r in refs)
    pipe = FlowPipeline(W, H, B, cfg, streams=slices)
    try:
        g = pipe.ctx.get_corner_grid()
        assert (g.cell, g.cap, g.max_rank) == grid
        pipe.upload(np.stack([q["prev"] for q in pairs]), np.stack([q["next"] for q in pairs]), sensors)
        for call in range(2):
            out = pipe.run()
            stats = pipe.corner_grid_stats()
            for b in range(B):
                assert_pair_matches(out, b, refs[b], f"grid slices {slices} call {call}")
                assert tuple(int(v) for v in stats[b]) == refs[b]["stats"], (b, stats[b], refs[b]["stats"])
    finally:
        pipe.close()


class ReplaceLoop:
    """The replace-mode loop (of_module.py:83-88 with the status keep rule): few tracks -> fresh corners of the previous frame through
    the grid, empty cells; then LK; tracks := the tracked points."""

    def __init__(self, first_frame, cfg, min_feat, grid):
        self.cfg, self.min_feat, self.grid = cfg, min_feat, grid
        self.g_prev = io.gray_bgr8(first_frame)
        self.tracks = self.detect(cfg.max_corners)

    def detect(self, k):
        c = self.cfg
        return R.good_features(self.g_prev, k, c.quality, c.min_distance, c.block_size, grid=self.grid)[0]

    def step(self, frame):
        cfg = self.cfg
        g = io.gray_bgr8(frame)
        old = self.tracks
        replaced = len(old) <= self.min_feat and cfg.max_corners - len(old) > 0
        if replaced:
            old = self.detect(cfg.max_corners - len(old))
        new, st = track(lambda a, b, o: io.lk_pyr(a, b, o, cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr), self.g_prev, g, old)
        self.tracks, self.g_prev = new[st == 1], g
        return dict(tracks=self.tracks.copy(), n_old=len(old), replaced=replaced)


# mode, grid, what the reference must show
STREAMS = [pytest.param("step", (40, 2, 0), "refills", id="step-cap2"), pytest.param("fused", (40, 2, 0), "refills", id="fused-cap2"),
           pytest.param("replace", (40, 1, 0), "replaces", id="replace-cap1"), pytest.param("step", (160, 3, 0), "full", id="step-cells-full")]


def stream_reference(ofk, mode, grid, shows):
    """Frames, sensors, configuration and the reference's answers of a stream case, with the checks that make the comparison mean
    something: the grid shapes what the streams hold."""
    from of_amd import synth
    from of_amd.pipeline import FusionConfig, FilterModel, PipelineConfig
    nf, B = 4, 2
    cfg = PipelineConfig(grid_cell=grid[0], grid_cap=grid[1], grid_max_rank=grid[2], **dict(CORNERS, max_corners=120), **LK)   # more than the cells hold
    seqs = [synth.render_sequence(H, W, 40 + b, nf, margin=160, **STREAM_MOTION) for b in range(B)]
    frames = np.stack([s[0] for s in seqs]).copy(); info = seqs[0][1]
    frames[1, 0] = 0                                             # the second stream starts on a blank frame: no old tracks when it first detects
    sensors = ofk.make_sensors(B, d=info["d"], normal=info["n"], omega=info["omega"], scaling=info["scaling"], cx=info["cx"], cy=info["cy"])
    min_feat, radius = cfg.max_corners, 8                        # every step re-detects
    fusion = None
    if mode == "fused":
        fusion = FusionConfig(use_imu=False, filter=True, z_sign=1.0, z_source=1, model=FilterModel.kf3())
    elif mode == "replace":
        fusion = FusionConfig(redetect_replace=True)
    if mode == "replace":
        loops = [ReplaceLoop(frames[b, 0], cfg, min_feat, grid) for b in range(B)]
        ref = [[loops[b].step(frames[b, t]) for b in range(B)] for t in range(1, nf)]
    else:
        loops = [R.GridNodeLoop(frames[b, 0], cfg, min_feat, radius, grid, **(dict(model=fusion.model) if fusion else {})) for b in range(B)]
        plain = [NodeLoop(frames[b, 0], cfg, min_feat, radius) for b in range(B)]
        ref = [[loops[b].step(frames[b, t], sensors[b]) for b in range(B)] for t in range(1, nf)]
        ref_plain = [[plain[b].step(frames[b, t], sensors[b]) for b in range(B)] for t in range(1, nf)]
    first = [R.good_features(io.gray_bgr8(frames[b, 0]), cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size, grid=grid)[0] for b in range(B)]
    assert len(first[0]) >= 10 and len(first[1]) == 0
    if shows == "refills":
        assert any(len(o["tracks"]) > o["n_tracked"] for row in ref for o in row)                       # re-detection added corners
        assert any(not np.array_equal(o["tracks"], q["tracks"]) for row, prow in zip(ref, ref_plain) for o, q in zip(row, prow))
        assert len(ref[1][1]["tracks"]) > 0 and ref[1][1]["n_old"] == 0                                 # ... also where there were no old tracks
    elif shows == "full":
        assert len(first[0]) == 4 * grid[1] and len(ref[0][0]["tracks"]) == ref[0][0]["n_tracked"]      # every cell full: nothing is added
        g0 = io.gray_bgr8(frames[0, 0])                          # ... where the disc mask alone leaves corners to add
        assert len(R.good_features(g0, cfg.max_corners - len(first[0]), cfg.quality, cfg.min_distance, cfg.block_size,
                                   mask=disc_mask(H, W, first[0], radius))[0]) > 0
    else:
        assert all(o["replaced"] for row in ref for o in row) and any(len(o["tracks"]) > 0 for o in ref[-1])
    return dict(cfg=cfg, frames=frames, sensors=sensors, fusion=fusion, min_feat=min_feat, radius=radius, first=first, ref=ref, nf=nf, B=B)


@pytest.mark.parametrize("mode,grid,shows", STREAMS)
def test_streams_redetect_through_the_grid(pkg, ofk, mode, grid, shows):
    from of_amd.pipeline import FlowStream
    c = stream_reference(ofk, mode, grid, shows)
    cfg, frames, sensors, fusion, min_feat, radius, first, ref, nf, B = (c[k] for k in ("cfg", "frames", "sensors", "fusion", "min_feat", "radius", "first", "ref", "nf", "B"))
    fs = FlowStream(W, H, batch=B, cfg=cfg, min_features=min_feat, mask_radius=radius, fusion=fusion)
    try:
        tracks, counts = fs.begin(frames[:, 0])
        for b in range(B):
            assert counts[b] == len(first[b]) and np.array_equal(bits(tracks[b, :counts[b]]), bits(first[b])), b
        for t in range(1, nf):
            if fusion:
                rec, fused, tracks, counts = fs.step_fused(frames[:, t], sensors)
            else:
                rec, tracks, counts = fs.step(frames[:, t], sensors)
            for b in range(B):
                o = ref[t - 1][b]; tag = (mode, grid, t, b)
                assert counts[b] == len(o["tracks"]) and rec[b, 12] == o["n_old"], (tag, counts[b], len(o["tracks"]), rec[b, 12], o["n_old"])
                assert np.array_equal(bits(tracks[b, :counts[b]]), bits(o["tracks"].astype(np.float32))), tag
    finally:
        fs.close()
