"""Test-side reference of the lighting-insensitive Lucas-Kanade (include/ofk.h: ofk_lk_light, ofk_lk_pyr_light).

lk_pyr       tests/lk_light_reference.c - lk_seed_reference.c restated with rules 1-6 of the header - compiled into a temporary
             directory with the oracle Makefile's flags; pyramids and Scharr derivatives come from oracle/image_oracle.py.
             light: None, "bias", "gain", or (mode, gain_max).
gated, gated_chain, gated_lk, seeded_gated_lk
             tests/track_gate_reference.py's compositions (the gates, the pair chain, the stream loop's tracker plugs) with this
             tracker in both passes.
experiment   the exposure experiment of the issue: rows of lk_seed_reference.ROWS with the next gray frame under another exposure.
"""
import atexit
import contextlib
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from oracle import image_oracle as io
import lk_seed_reference as R  # tests/lk_seed_reference.py
import track_gate_reference as G  # tests/track_gate_reference.py

_HERE = os.path.dirname(os.path.abspath(__file__))
OFF, BIAS, GAIN = 0, 1, 2
MODES = {"off": OFF, "bias": BIAS, "gain": GAIN}
GAIN_MAX = 4.0
_lib = None


def _load():
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="lk_light_ref_")
        atexit.register(shutil.rmtree, tmp, True)
        so = os.path.join(tmp, "liblklightref.so")
        subprocess.check_call([os.environ.get("CC", "gcc")] + R._CFLAGS + ["-shared", "-o", so, os.path.join(_HERE, "lk_light_reference.c"), "-lm"])
        L = C.CDLL(so)
        pp = C.POINTER(C.c_void_p)
        L.ref_lk_light.argtypes = [pp, pp, pp, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                   C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def light_of(light):
    """None / "off" / "bias" / "gain" / (mode, gain_max) / an object with .mode and .gain_max -> (mode, gain_max)."""
    if light is None:
        return OFF, GAIN_MAX
    if isinstance(light, str):
        return MODES[light], GAIN_MAX
    if hasattr(light, "mode"):
        return int(light.mode), float(light.gain_max)
    mode, gmax = light
    return (MODES[mode] if isinstance(mode, str) else int(mode)), float(gmax)


def lk_pyr(prev, nxt, prev_pts, win=15, max_level=3, max_count=20, eps=0.03, min_eig_thr=1e-4, seed=None, flags=0, light=None, iters=False):
    """lk_seed_reference.lk_pyr's signature plus light.  -> (next (N,1,2) f32, status (N,1) u8, err (N,1) f32[, Newton steps])."""
    mode, gmax = light_of(light)
    prev = np.ascontiguousarray(prev, np.uint8); nxt = np.ascontiguousarray(nxt, np.uint8)
    if not (win >= 3 and win <= 31 and win & 1 and 0 <= max_level <= 8):
        raise ValueError("lk_pyr: bad window or level")
    P = io.pyramid(prev, win, max_level); Q = io.pyramid(nxt, win, max_level)
    D = [io.scharr(a) for a in P]
    L = len(P) - 1
    p = np.ascontiguousarray(prev_pts, np.float32).reshape(-1, 2)
    n = len(p)
    sd = None
    if flags & R.USE_INITIAL_FLOW:
        sd = np.ascontiguousarray(seed, np.float32).reshape(-1, 2)
        assert sd.shape == p.shape
    hs = np.array([a.shape[0] for a in P], np.int32); ws = np.array([a.shape[1] for a in P], np.int32)
    out = np.zeros((n, 2), np.float32); st = np.zeros(n, np.uint8); err = np.zeros(n, np.float32)
    it = np.zeros((n, 9), np.int32) if iters else None

    def ptrs(arrs):
        return (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])

    rc = _load().ref_lk_light(ptrs(P), ptrs(Q), ptrs(D), hs.ctypes.data, ws.ctypes.data, L, p.ctypes.data,
                              sd.ctypes.data if sd is not None else None, n, int(win), int(max_count), float(eps), float(min_eig_thr),
                              int(flags), mode, gmax, out.ctypes.data, st.ctypes.data, err.ctypes.data, it.ctypes.data if iters else None)
    if rc:
        raise ValueError(f"ref_lk_light rc={rc}")
    res = (out.reshape(n, 1, 2), st.reshape(n, 1), err.reshape(n, 1))
    return res + (it,) if iters else res


class _Tracker:
    """What tests/track_gate_reference.py reads of lk_seed_reference, with this module's tracker under a fixed light."""
    USE_INITIAL_FLOW = R.USE_INITIAL_FLOW
    predict = staticmethod(R.predict)

    def __init__(self, light):
        self.light = light

    def lk_pyr(self, *a, **kw):
        return lk_pyr(*a, light=self.light, **kw)


@contextlib.contextmanager
def under(light):
    """track_gate_reference's rules with the forward and the backward pass under `light`: the rules themselves stay that module's."""
    saved = G.R
    G.R = _Tracker(light)
    try:
        yield
    finally:
        G.R = saved


def gated(g0, g1, pts, win, max_level, max_count, eps, min_eig_thr, gate, seed=None, flags=0, light=None):
    """track_gate_reference.gated under `light` (gate G.OFF: the tracker alone, keep = its status)."""
    with under(light):
        return G.gated(g0, g1, pts, win, max_level, max_count, eps, min_eig_thr, gate, seed=seed, flags=flags)


def gated_chain(prev, nxt, cfg, sr, gate, light):
    """track_gate_reference.gated_chain under `light`: corners -> LK (and the gates) -> the NODE solve, for one BGR pair."""
    with under(light):
        return G.gated_chain(prev, nxt, cfg, sr, gate)


def gated_lk(cfg, gate, light, log=None):
    """The tracker plug lk(g_prev, g, old) of stream_oracle.NodeLoop under `light`."""
    inner = G.gated_lk(cfg, gate, log)

    def lk(g_prev, g, old):
        with under(light):
            return inner(g_prev, g, old)
    return lk


def seeded_gated_lk(cfg, gate, mode, light, gain=1.0, log=None, predict=None):
    """NodeLoop's lk_src plug under ofk_set_lk_seed + ofk_set_track_gate + ofk_set_lk_light."""
    inner = G.seeded_gated_lk(cfg, gate, mode, gain, log, predict)

    def lk(g_prev, g, old, src):
        with under(light):
            return inner(g_prev, g, old, src)
    return lk


# ---------------------------------------------------------------------------------------- the exposure experiment
# (gain, bias, vignette) of the issue's table, in its order
EXPOSURES = ((1.0, 0.0, 0.0), (1.25, 10.0, 0.0), (0.75, -5.0, 0.0), (1.1, 0.0, 0.0), (1.25, 10.0, 0.3))
_exposed = {}


def exposed_g1(name, exposure):
    """The next gray frame of lk_seed_reference.experiment_pair(name) under (gain, bias, vignette)."""
    key = (name, tuple(exposure))
    if key not in _exposed:
        from of_amd import synth
        _exposed[key] = synth.apply_exposure(R.experiment_pair(name)["g1"], *exposure)
    return _exposed[key]


def experiment_row(name, exposure, light):
    """-> dict(tracked, wrong, right, rel, dist, err): status-1 points, of those more than 0.5 px from the true end point, the rest,
    track_gate_reference.node_rel_error on the tracked points, the median distance of the tracked points from their true end point
    and the median err of the right ones."""
    e = R.experiment_pair(name)
    nxt, st, err = lk_pyr(e["g0"], exposed_g1(name, exposure), e["pts"], max_level=3, light=light, **R.EXP_LK)
    nxt = nxt.reshape(-1, 2); tracked = st.ravel() == 1
    d = np.linalg.norm(nxt.astype(np.float64) - (e["pts"].astype(np.float64) + e["flow"]), axis=1)
    right = tracked & (d <= 0.5)
    return dict(tracked=int(tracked.sum()), wrong=int((tracked & ~right).sum()), right=int(right.sum()),
                rel=G.node_rel_error(e, nxt, tracked) if tracked.sum() >= 3 else float("nan"),
                dist=float(np.median(d[tracked])) if tracked.any() else float("nan"),
                err=float(np.median(err.ravel()[right])) if right.any() else float("nan"))
