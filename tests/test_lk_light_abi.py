"""The lighting-insensitive LK's entry points exist in the header, the binding and the library; the setting's structure agrees on both
sides; the kernels are in the code object; lk_light_setting's defaults and every invalid field; the pipeline configuration and
optical_fusion carry the setting; light=None never reaches the new entry; synth.apply_exposure is the stated formula (CPU-only).
On a device: the setting's default, its round trip, every refusal leaving the setting as it was, and off after NULL."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_lk_light", "ofk_get_lk_light", "ofk_lk_pyr_light")
FIELDS = ["mode", "gain_max"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge


def values(m):
    return [getattr(m, n) for n in FIELDS]


def test_entry_points_declared_bound_and_exported(built, ofk):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofk.h")).read(), flags=re.S)
    lib = ofk.load_library()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert s in ofk.SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
    for name, val in (("OFK_LIGHT_OFF", 0), ("OFK_LIGHT_BIAS", 1), ("OFK_LIGHT_GAIN", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
    assert (ofk.LIGHT_OFF, ofk.LIGHT_BIAS, ofk.LIGHT_GAIN) == (0, 1, 2)
    assert ofk.LIGHT_MODES == {"off": 0, "bias": 1, "gain": 2}
    m = re.search(r"typedef struct ofk_lk_light \{(.*?)\} ofk_lk_light;", txt, flags=re.S)
    assert m and [n for _, n in re.findall(r"\b(int|double)\s+(\w+);", m.group(1))] == FIELDS
    assert [n for n, _ in ofk.LkLight._fields_] == FIELDS
    assert [t for _, t in ofk.LkLight._fields_] == [C.c_int, C.c_double]
    assert C.sizeof(ofk.LkLight) == 16 and ofk.LkLight.gain_max.offset == 8
    # ofk_lk_pyr_fb's argument list plus the light
    assert lib.ofk_lk_pyr_light.argtypes[:-1] == lib.ofk_lk_pyr_fb.argtypes and len(lib.ofk_lk_pyr_light.argtypes) == 24
    fb = re.search(r"int ofk_lk_pyr_fb\((.*?)\);", txt, flags=re.S).group(1)
    light = re.search(r"int ofk_lk_pyr_light\((.*?)\);", txt, flags=re.S).group(1)
    norm = lambda a: [" ".join(p.split()) for p in a.split(",")]
    assert norm(light) == norm(fb) + ["const ofk_lk_light *light"]
    assert lib.ofk_set_lk_light(None, None) == ofk.E_INVALID and lib.ofk_get_lk_light(None, None) == ofk.E_INVALID


def test_light_kernels_are_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for wmax in (15, 21, 31):
        for flags in (0, 4, 8, 12):
            assert b"k_lk_lightILi%dELi%dEE" % (wmax, flags) in blob, (wmax, flags)
    for k in (b"k_lk15q", b"k_lk15_fILi4EE", b"k_lk_fILi31ELi12EE"):     # the existing trackers are still there
        assert k in blob, k


def test_settings_from_names(built, ofk):
    assert values(ofk.lk_light_setting()) == [2, 4.0]
    assert values(ofk.lk_light_setting("bias")) == [1, 4.0]
    assert values(ofk.lk_light_setting(ofk.LIGHT_GAIN, 1.5)) == [2, 1.5]
    assert ofk.lk_light_setting("off").mode == 0
    nan, inf = float("nan"), float("inf")
    for bad in (dict(mode="contrast"), dict(mode=3), dict(mode=-1), dict(gain_max=1.0), dict(gain_max=0.5), dict(gain_max=-4.0),
                dict(gain_max=nan), dict(gain_max=inf), dict(gain_max=-inf)):
        with pytest.raises(ValueError):
            ofk.lk_light_setting(**bad)
    with pytest.raises(TypeError):
        ofk.lk_light_setting(gain_min=0.5)


class Recorder:
    """Stands in for ofk.Context: records what a pipeline applies to it."""
    calls = []

    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        def f(*a, **k):
            Recorder.calls.append((name, a, k))
        return f


def test_pipeline_config_carries_the_setting(built, pkg, ofk, monkeypatch):
    from of_amd import pipeline
    from of_amd.pipeline import PipelineConfig, FlowPipeline, FlowStream
    for cfg in (PipelineConfig(), PipelineConfig.node(), PipelineConfig.of_module(), PipelineConfig.evaluate_exp(), PipelineConfig.baseline_1080p()):
        assert cfg.lk_light is None and cfg.lk_light_setting() is None
    assert values(PipelineConfig(lk_light="gain").lk_light_setting()) == [2, 4.0]
    assert values(PipelineConfig(lk_light="bias").lk_light_setting()) == [1, 4.0]
    given = ofk.lk_light_setting("gain", 2.5)
    on = PipelineConfig(lk_light=given)
    assert values(on.lk_light_setting()) == [2, 2.5]
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params())          # to_params() does not know the setting
    assert PipelineConfig(lk_light="off").lk_light_setting() is None
    assert PipelineConfig(lk_light=ofk.lk_light_setting("off")).lk_light_setting() is None
    for bad in (ofk.LkLight(2, 1.0), ofk.LkLight(7, 4.0), "contrast", 2.5, True):
        with pytest.raises(ValueError):
            PipelineConfig(lk_light=bad).lk_light_setting()
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    Recorder.calls = []
    FlowStream(64, 48, batch=1, cfg=PipelineConfig())
    FlowPipeline(64, 48, batch=1, cfg=PipelineConfig())
    assert not [c for c in Recorder.calls if c[0] == "set_lk_light"]
    FlowStream(64, 48, batch=1, cfg=on)
    FlowPipeline(64, 48, batch=1, cfg=on)
    sets = [c for c in Recorder.calls if c[0] == "set_lk_light"]
    assert len(sets) == 2 and all(values(c[1][0]) == [2, 2.5] for c in sets)


def test_optical_fusion_hands_the_setting_to_its_pipeline_config(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    from of_amd.velocity_node import optical_fusion
    assert optical_fusion(spin=False)._lk_light == {}
    assert optical_fusion(spin=False, lk_light=False)._lk_light == {}
    node = optical_fusion(spin=False, lk_light="gain")
    assert values(PipelineConfig(**node._lk_light).lk_light_setting()) == [2, 4.0]
    node = optical_fusion(spin=False, lk_light=dict(mode="bias", gain_max=2.0))
    assert values(PipelineConfig(**node._lk_light).lk_light_setting()) == [1, 2.0]
    given = ofk.lk_light_setting("gain", 3.0)
    assert optical_fusion(spin=False, lk_light=given)._lk_light["lk_light"] is given
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, lk_light=dict(gain_max=1.0))
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, lk_light=dict(gain_min=3))
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, lk_light="contrast")


class FakeLib:
    """Stands in for libofk.so behind Context.lk_pyr / lk_pyr_fb: records which entry a call reaches."""
    def __init__(self):
        self.reached = []

    def __getattr__(self, name):
        def f(*a):
            self.reached.append((name, len(a)))
            return 0
        return f


def test_light_none_never_reaches_the_new_entry(built, ofk):
    import threading
    ctx = ofk.Context.__new__(ofk.Context)
    ctx._L = FakeLib(); ctx._h = None; ctx._lock = threading.RLock(); ctx.max_batch = 4; ctx.max_pts = 16
    ctx._ck = lambda rc: None
    g = np.zeros((2, 48, 64), np.uint8)
    pts = np.zeros((2, 4, 2), np.float32)
    counts = [4, 2]
    for light in (None, "off", ofk.lk_light_setting("off"), ofk.LkLight(0, 4.0)):
        ctx.lk_pyr(g, g, pts, counts, light=light)
        ctx.lk_pyr(g, g, pts, counts, next_pts=pts, flags=ofk.LK_USE_INITIAL_FLOW, light=light)
        ctx.lk_pyr_fb(g, g, pts, counts, fb="plain", light=light)
    assert [n for n, _ in ctx._L.reached] == ["ofk_lk_pyr", "ofk_lk_pyr_ex", "ofk_lk_pyr_fb"] * 4
    ctx._L.reached.clear()
    for light in ("bias", "gain", ofk.lk_light_setting("gain", 2.0)):
        ctx.lk_pyr(g, g, pts, counts, light=light)
        ctx.lk_pyr_fb(g, g, pts, counts, fb="plain", light=light)
    assert ctx._L.reached == [("ofk_lk_pyr_light", 24)] * 6
    for bad in ("contrast", ofk.LkLight(2, 0.5), 1.5):
        with pytest.raises(ValueError):
            ctx.lk_pyr(g, g, pts, counts, light=bad)
    ctx._h = None                                                # nothing to close


def test_apply_exposure_is_the_stated_formula(pkg):
    from of_amd import synth
    rng = np.random.default_rng(5)
    h, w = 37, 52
    gray = rng.integers(0, 256, (h, w), dtype=np.uint8)
    bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    assert np.array_equal(synth.apply_exposure(gray), gray) and np.array_equal(synth.apply_exposure(bgr), bgr)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    r2 = ((xx - w / 2) ** 2 + (yy - h / 2) ** 2) / ((w / 2) ** 2 + (h / 2) ** 2)
    for gain, bias, vig in ((1.25, 10.0, 0.0), (0.75, -5.0, 0.3), (6.0, 0.0, 0.0), (1.0, -300.0, 0.0)):
        want = np.clip(np.rint(gray * gain * (1 - vig * r2) + bias), 0, 255).astype(np.uint8)
        got = synth.apply_exposure(gray, gain, bias, vig)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (gain, bias, vig)
        got3 = synth.apply_exposure(bgr, gain, bias, vig)
        assert got3.shape == bgr.shape and all(np.array_equal(got3[..., c], synth.apply_exposure(bgr[..., c].copy(), gain, bias, vig)) for c in range(3))
    assert synth.apply_exposure(gray, 6.0).max() == 255 and synth.apply_exposure(gray, 1.0, -300.0).max() == 0
    assert r2[0, 0] == 1.0                                      # the corner pixel sees the whole vignette
    with pytest.raises(ValueError):
        synth.apply_exposure(gray.astype(np.float32))


@pytest.mark.gpu
def test_setting_round_trip_every_refusal_and_off_after_null(pkg, ofk):
    ctx = ofk.Context(0, 64, 48, 2, 100, 2)
    try:
        assert values(ctx.get_lk_light()) == [0, 4.0]              # off, the default clamp
        good = ofk.LkLight(2, 2.5)
        ctx.set_lk_light(good)
        assert values(ctx.get_lk_light()) == [2, 2.5]
        nan, inf = float("nan"), float("inf")
        for bad in ((3, 2.5), (-1, 2.5), (2, 1.0), (1, 0.5), (2, -4.0), (2, nan), (1, inf), (2, -inf)):
            with pytest.raises(ofk.OfkError) as e:
                ctx.set_lk_light(ofk.LkLight(*bad))
            assert e.value.code == ofk.E_INVALID, bad
            assert values(ctx.get_lk_light()) == [2, 2.5], bad                           # the previous setting is in place
        ctx.set_lk_light("bias")
        assert values(ctx.get_lk_light()) == [1, 4.0]
        ctx.set_lk_light(None)
        assert values(ctx.get_lk_light()) == [0, 4.0]
        ctx.set_lk_light(mode="gain", gain_max=3.0)
        ctx.set_lk_light(ofk.LkLight(0, nan))                      # mode off: off, whatever else it holds
        assert values(ctx.get_lk_light()) == [0, 3.0]
        ctx.set_lk_light("gain", gain_max=8.0)
        assert values(ctx.get_lk_light()) == [2, 8.0]
        ctx.set_lk_light("off")
        assert ctx.get_lk_light().mode == 0
    finally:
        ctx.close()
