#!/usr/bin/env python3
"""Generates tests/golden/jpeg_edges.npz: the JPEG streams at the two edges of the device decoder (k_jpeg.hip) that the textured
frames of jpeg_golden.npz never reach, each with the BGR pixels libjpeg-turbo's default decompressor returned for it (through
Pillow: Image.open(...).convert("RGB")[..., ::-1], a gray plane replicated over the channels - the cv2.IMREAD_COLOR layout).  The
expectation is libjpeg's, not the oracle's.

  slow streams   periodic or flat content, whose chunk decoders never fall into step by themselves: the truth advances one chunk
                 per synchronisation pass (tests/jpeg_sync_model.py chooses the sizes; `cond_*` records the pass-count condition
                 every one of them was chosen for, at 64-byte chunks, and tests/test_jpeg_sync_model.py holds them to it);
  tiny frames    1x1 ... 24x40 in every sampling, from noise and from a flat colour: one MCU, a single chunk, chroma planes of one
                 or two samples (where libjpeg replicates instead of filtering).

Inputs come from seeded generators and of_amd.synth alone.  Layout (one blob per kind, so that the streams' identical headers
compress together): names[N]; jpg = the streams back to back, jpg_off[N + 1]; bgr = the pixels back to back in the same order,
shape[N] = (h, w).  Run once in the build container:  python tests/golden/make_golden_jpeg_edges.py
"""
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TINY_SIZES = [(1, 1), (1, 2), (2, 1), (3, 3), (7, 5), (8, 8), (9, 8), (8, 9), (15, 17), (16, 16), (17, 16), (16, 17), (1, 33), (33, 1),
              (2, 35), (31, 2), (24, 40)]                         # (h, w)
TINY_MODES = [("gray", None), ("444", 0), ("422", 1), ("420", 2)]
TINY_FLAT = (200, 60, 30)                                        # RGB


def encode(img, quality, subsampling=None, **extra):
    buf = io.BytesIO()
    kw = {} if subsampling is None else {"subsampling": subsampling}
    kw.update(extra)
    Image.fromarray(img).save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def decode_bgr(data):
    im = Image.open(io.BytesIO(data))
    if im.mode == "L":
        return np.repeat(np.asarray(im)[:, :, None], 3, axis=2)
    return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def stripes(h, w):
    """Vertical stripes, period 8 pixels (= one block), values 20 / 220."""
    row = np.where((np.arange(w) // 4) % 2 == 0, 20, 220).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(row[None, :, None], (h, w, 3)))


def flat(h, w, v, gray=False):
    return np.full((h, w) if gray else (h, w, 3), v, np.uint8)


def main():
    import jpeg_sync_model as model
    from __graft_entry__ import load_package
    load_package()
    from of_amd import synth

    entries, cond = [], []                                       # (name, stream); (name, lowest, highest modelled pass count)

    def add(name, data, lo=None, hi=None):
        entries.append((name, data))
        if lo is not None:
            cond.append((name, lo, hi))

    # ---- slow streams (quality 80, the default of compressed_image_transport).  Stripes 4:4:4: one stream per look window of the
    # host loop around the boundary of its 64 flag slots (it looks after passes 7, 11, ..., 59, 63, 67, 71), two far behind it.
    BIG = 1 << 30
    for (h, w), (lo, hi) in [((64, 320), (56, 59)), ((72, 304), (60, 63)), ((72, 320), (64, 67)), ((80, 312), (68, 71)),
                             ((160, 320), (128, BIG)), ((240, 320), (128, BIG))]:
        add(f"stripes_{h}x{w}", encode(stripes(h, w), 80, 0), lo, hi)
    add("stripes_72x320_rst", encode(stripes(72, 320), 80, 0, restart_marker_rows=1))      # (restart intervals: outside the model)
    add("black_480x640_420", encode(flat(480, 640, 0), 80, 2), 64, BIG)
    add("white_480x640_420", encode(flat(480, 640, 255), 80, 2), 64, BIG)
    add("black_1080x1920_420", encode(flat(1080, 1920, 0), 80, 2), 128, BIG)
    # fitted tables of a flat frame: one-bit codes, the bit stream is all zeros
    add("opt_gray_240x320", encode(flat(240, 320, 128, gray=True), 80, None, optimize=True))
    add("opt_444_240x320", encode(flat(240, 320, 128), 80, 0, optimize=True))
    add("opt_420_240x320", encode(flat(240, 320, 128), 80, 2, optimize=True))
    # textured frames of the slow 72x320 stream's geometry, for batches that mix both kinds
    for k in range(2):
        add(f"tex_72x320_{'ab'[k]}", encode(np.ascontiguousarray(synth.render_pair(72, 320, 900 + k)["prev"]), 80, 0))

    # ---- tiny frames (quality 90): noise, a flat colour, other noise - three streams of different content per geometry
    rng = np.random.default_rng(20240607)
    for h, w in TINY_SIZES:
        for mode, ss in TINY_MODES:
            for content in ("noise", "flat", "noise2"):
                if content == "flat":
                    img = np.empty((h, w, 3), np.uint8); img[:] = TINY_FLAT
                else:
                    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
                if ss is None:
                    img = np.ascontiguousarray(img[:, :, 1])
                add(f"tiny_{h}x{w}_{mode}_{content}", encode(img, 90, ss))

    for name, lo, hi in cond:                                    # the conditions hold when the file is made; the CPU suite re-checks them
        n = model.passes(dict(entries)[name], 64)[1]
        assert lo <= n <= hi, (name, n, lo, hi)
    pix = [decode_bgr(d) for _, d in entries]
    out = {
        "libjpeg": np.array(f"libjpeg-turbo {features.version('libjpeg_turbo')} via Pillow {PIL.__version__}"),
        "names": np.array([n for n, _ in entries]),
        "jpg": np.frombuffer(b"".join(d for _, d in entries), np.uint8),
        "jpg_off": np.cumsum([0] + [len(d) for _, d in entries]).astype(np.int64),
        "bgr": np.concatenate([p.ravel() for p in pix]),
        "shape": np.array([p.shape[:2] for p in pix], np.int32),
        "cond_names": np.array([c[0] for c in cond]),
        "cond_lo": np.array([c[1] for c in cond], np.int64),
        "cond_hi": np.array([c[2] for c in cond], np.int64),
    }
    path = os.path.join(HERE, "jpeg_edges.npz")
    np.savez_compressed(path, **out)
    print(len(entries), "streams,", out["jpg"].size, "stream bytes,", out["bgr"].size, "pixel bytes ->", os.path.getsize(path), "bytes;", str(out["libjpeg"]))


if __name__ == "__main__":
    main()
