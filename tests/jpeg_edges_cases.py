"""Reader of tests/golden/jpeg_edges.npz (tests/golden/make_golden_jpeg_edges.py): slow-synchronising and tiny JPEG streams with
the pixels libjpeg returned for them.  Shared by the CPU and the GPU tests; needs neither Pillow nor a GPU."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_edges.npz")

TINY_SIZES = [(1, 1), (1, 2), (2, 1), (3, 3), (7, 5), (8, 8), (9, 8), (8, 9), (15, 17), (16, 16), (17, 16), (16, 17), (1, 33), (33, 1),
              (2, 35), (31, 2), (24, 40)]                         # (h, w): the sizes the fixture file must hold
TINY_MODES = ("gray", "444", "422", "420")
TINY_CONTENTS = ("noise", "flat", "noise2")


class Edges:
    def __init__(self, path=PATH):
        z = np.load(path)
        self.libjpeg = str(z["libjpeg"])
        self.names = [str(n) for n in z["names"]]
        self._index = {n: i for i, n in enumerate(self.names)}
        self._jpg, self._joff = z["jpg"], z["jpg_off"]
        self._bgr, self._shape = z["bgr"], z["shape"]
        self._boff = np.concatenate([[0], np.cumsum(self._shape[:, 0].astype(np.int64) * self._shape[:, 1] * 3)])
        self._bgr.setflags(write=False)
        self.conditions = {str(n): (int(lo), int(hi)) for n, lo, hi in zip(z["cond_names"], z["cond_lo"], z["cond_hi"])}

    def jpg(self, name):
        i = self._index[name]
        return self._jpg[self._joff[i]:self._joff[i + 1]].tobytes()

    def bgr(self, name):
        """[h][w][3] uint8, a read-only view."""
        i = self._index[name]
        h, w = self._shape[i]
        return self._bgr[self._boff[i]:self._boff[i + 1]].reshape(h, w, 3)

    def tiny(self, h, w, mode):
        """names of the three streams of one tiny geometry"""
        return [f"tiny_{h}x{w}_{mode}_{c}" for c in TINY_CONTENTS]


def narrow_chroma(h, w, mode):
    """libjpeg (jdsample.c jinit_upsampler) filters a horizontally subsampled plane only when it is more than two samples wide."""
    return mode in ("422", "420") and (w + 1) // 2 <= 2
