"""The device JPEG decoder (k_jpeg.hip) where its textured test frames never take it, against the pixels libjpeg returned
(tests/golden/jpeg_edges.npz - committed streams and pixels: nothing here needs Pillow, nothing skips without it).

Slow streams: periodic and flat content keeps a misaligned chunk decoder in a stable wrong cycle, so the truth advances one chunk per
synchronisation pass and the host loop of jdecode_staged runs for as many passes as the stream has chunks - through its 64 flag
slots, into the reuse of the last one, with the memset between the tail passes.  tests/jpeg_sync_model.py says which stream takes
how long (tests/test_jpeg_sync_model.py holds the fixtures to that); the device is asked for the right PIXELS, and, through
ofk_jpeg_last_iterations, for proof that it went where the test means it to go.

Tiny frames: one MCU, a single chunk (no synchronisation at all), planes narrower than an upsampling tile, and chroma planes of one
or two samples, which libjpeg replicates instead of filtering."""
import numpy as np
import pytest

from jpeg_edges_cases import Edges, TINY_SIZES, TINY_MODES, narrow_chroma

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def edges():
    return Edges()


@pytest.fixture
def chunk64(ofk):
    """64 entropy bytes per decoder thread, whatever the batch would choose: the chunk size the model's pass counts are for"""
    ofk.set_tuning("jpeg_chunk", 64)
    try:
        yield
    finally:
        ofk.set_tuning("jpeg_chunk", 0)


def _check(ctx, edges, names):
    out = ctx.jpeg_decode([edges.jpg(n) for n in names])
    assert out.shape[0] == len(names)
    for k, n in enumerate(names):
        assert out[k].shape == edges.bgr(n).shape, (k, n)
        assert np.array_equal(out[k], edges.bgr(n)), (k, n, names)
    return ctx.jpeg_last_iterations()


# ------------------------------------------------------------------------------------------------ slow streams
@pytest.mark.parametrize("name", ["stripes_64x320", "stripes_72x304", "stripes_72x320", "stripes_80x312"])
def test_stripes_around_the_last_flag_slot(gpu_ctx, edges, chunk64, name):
    """Modelled fixed points at passes 58, 62, 65 and 70: one in each of the host's looks at the flags around slot 63 (it looks after
    passes 59, 63, 67 and 71) - the last burst inside the slots, the one that ends ON the reused slot, the first and the second
    that live in it alone."""
    lo, hi = edges.conditions[name]
    assert 56 <= lo and hi <= 71
    n = _check(gpu_ctx, edges, [name])
    print(f"{name}: modelled fixed point in passes {lo}..{hi}, device queued {n}")


@pytest.mark.parametrize("name", ["stripes_160x320", "stripes_240x320"])
def test_streams_far_behind_the_flag_slots(gpu_ctx, edges, chunk64, name):
    """145 and 217 modelled passes: right pixels, no "did not converge", and the loop did go past its 64 slots.  (The host loop
    model rounds the fixed points up to the end of their bursts of four: 147 and 219 passes queued.  Counts on the device: not seen yet.)"""
    assert edges.conditions[name][0] >= 128
    n = _check(gpu_ctx, edges, [name])
    print(f"{name}: device queued {n} passes")
    assert n > 64, n


@pytest.mark.parametrize("name", ["black_480x640_420", "white_480x640_420", "black_1080x1920_420"])
def test_flat_frames_at_the_default_chunking(gpu_ctx, edges, name):
    """Lens cap and saturated sky: 76 chunks / 76 modelled passes at 480x640, 511 / 511 for the 1080p frame - a single frame is cut
    into 64-byte chunks by default.  (The host loop model queues 79 passes at 480x640 and 511 at 1080p.  Counts on the device: not seen yet.)"""
    n = _check(gpu_ctx, edges, [name])
    print(f"{name}: device queued {n} passes")
    assert n > 0


def test_fitted_one_bit_tables(gpu_ctx, edges, chunk64):
    """optimize=True on flat frames (gray, 4:4:4, 4:2:0): every code is one bit, the bit stream all zeros - the first-level table's
    shortest entries and, in the padding behind the data, the same zeros again."""
    for name in ("opt_gray_240x320", "opt_444_240x320", "opt_420_240x320"):
        _check(gpu_ctx, edges, [name])
        _check(gpu_ctx, edges, [name] * 3)


@pytest.mark.parametrize("order", [("tex_72x320_a", "stripes_72x320", "tex_72x320_b"), ("stripes_72x320", "tex_72x320_a", "tex_72x320_b")])
def test_one_slow_stream_keeps_the_batch_iterating(gpu_ctx, edges, chunk64, order):
    """The convergence flags belong to the batch: textured streams (fixed point inside the first burst) sit through the 65 passes of
    the stripes beside them and must come out untouched, whichever image the slow one is."""
    n = _check(gpu_ctx, edges, list(order))
    assert n > 16, n                                             # the textured streams alone need fewer (tests/test_jpeg_sync_model.py)
    assert _check(gpu_ctx, edges, ["tex_72x320_a", "tex_72x320_b"]) <= 16


def test_chunk_size_does_not_change_the_pixels_of_a_slow_stream(gpu_ctx, ofk, edges):
    seen = {}
    try:
        for chunk in (64, 128, 256, 1024, 0):
            ofk.set_tuning("jpeg_chunk", chunk)
            seen[chunk] = _check(gpu_ctx, edges, ["stripes_160x320"])
    finally:
        ofk.set_tuning("jpeg_chunk", 0)
    print("stripes_160x320: passes queued per chunk size", seen)
    assert seen[64] > 64 and seen[0] == seen[64]                 # (one small stream: the default is the smallest chunk)


def test_restart_variant_beside_the_slow_stream(gpu_ctx, edges, chunk64):
    """The same stripes with a restart marker per MCU row (every decoder is in step from the next marker on) in one batch with the
    marker-less stream: the restart instantiation of the tail pass on a batch in which one image still iterates."""
    _check(gpu_ctx, edges, ["stripes_72x320_rst", "stripes_72x320"])
    n = _check(gpu_ctx, edges, ["stripes_72x320", "stripes_72x320_rst", "stripes_72x320"])
    assert n > 16, n
    _check(gpu_ctx, edges, ["stripes_72x320_rst"])


def test_truncated_slow_stream_is_an_error_not_a_spin(gpu_ctx, ofk, edges, chunk64):
    """Half the entropy data of the flat black frame, then EOI: the decoders of what is left still need a pass per chunk, the fixed
    point exists, and the error is the one of a textured stream cut short - not the non-convergence guard."""
    data = edges.jpg("black_480x640_420")
    sos = data.index(b"\xff\xda")
    e0 = sos + 2 + ((data[sos + 2] << 8) | data[sos + 3])
    cut = data[:e0 + (len(data) - 2 - e0) // 2] + b"\xff\xd9"
    assert ofk.jpeg_info(cut) == (480, 640, 3) and len(ofk.jpeg_destuff(cut)[0]) > 20 * 64
    with pytest.raises(ofk.OfkError, match="truncated|corrupt"):
        gpu_ctx.jpeg_decode([cut])
    assert 16 < gpu_ctx.jpeg_last_iterations() < 76
    with pytest.raises(ofk.OfkError, match="truncated|corrupt"):
        gpu_ctx.jpeg_decode([data, cut])
    _check(gpu_ctx, edges, ["black_480x640_420"])


@pytest.mark.parametrize("prev,nxt", [("stripes_72x320", "tex_72x320_a"), ("black_480x640_420", "white_480x640_420")])
def test_gray_direct_ingest_behind_a_long_sync_loop(pkg, ofk, edges, prev, nxt):
    """ofk_pairs_upload_jpeg (the colour kernel writes gray level 0 of the resident pyramids, on the ingest stream) with a slow
    previous frame - stripes beside a textured next frame, a flat black frame beside a flat white one: the resident pyramids equal
    those of the fixture pixels uploaded raw, and so does everything the pipeline makes of them (nothing, on the flat pair)."""
    from of_amd.pipeline import FlowPipeline, PipelineConfig
    h, w, _ = edges.bgr(prev).shape
    pipe = FlowPipeline(w, h, 1, PipelineConfig(max_corners=60, quality=0.03, min_distance=7, max_level=2))
    try:
        sensors = ofk.make_sensors(1, scaling=0.002, cx=w / 2, cy=h / 2)
        pipe.upload(np.ascontiguousarray(edges.bgr(prev))[None], np.ascontiguousarray(edges.bgr(nxt))[None], sensors)
        ref = pipe.run()
        ref_pyr = [pipe.ctx.resident_pyramid(s, 0, h, w, 2) for s in (0, 1)]
        pipe.ctx.pairs_upload_jpeg([edges.jpg(prev)], [edges.jpg(nxt)])
        assert pipe.ctx.jpeg_last_iterations() > 64
        out = pipe.run()
        got_pyr = [pipe.ctx.resident_pyramid(s, 0, h, w, 2) for s in (0, 1)]
        for s in (0, 1):
            for l in range(3):
                assert np.array_equal(got_pyr[s][l], ref_pyr[s][l]), (s, l)
        for k in ("counts", "prev_pts", "next_pts", "status", "records"):
            assert np.array_equal(out[k], ref[k], equal_nan=True) if out[k].dtype.kind == "f" else np.array_equal(out[k], ref[k]), k
    finally:
        pipe.close()


# ------------------------------------------------------------------------------------------------ tiny frames
@pytest.mark.parametrize("h,w", TINY_SIZES)
def test_tiny_frames(ofk, edges, h, w):
    """Every sampling of one size as a batch of three streams of different content (noise, a flat colour, other noise), in a context
    of the frame's size - or of 16 pixels where the frame is smaller: ofk_create takes no smaller limits.  A batch whose streams fit
    one 64-byte chunk each queues no synchronisation pass; any other queues the first burst at least."""
    ctx = ofk.Context(0, max(w, 16), max(h, 16), 3, 64, 1)
    try:
        assert ctx.jpeg_last_iterations() == 0                   # before any decode
        for mode in TINY_MODES:
            names = edges.tiny(h, w, mode)
            single = all(len(ofk.jpeg_destuff(edges.jpg(n))[0]) < 64 for n in names)
            n = _check(ctx, edges, names)
            assert (n == 0) if single else (n >= 7), (mode, single, n, narrow_chroma(h, w, mode))
            _check(ctx, edges, names[1:2])                      # the flat stream alone
    finally:
        ctx.close()
