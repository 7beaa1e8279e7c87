"""The exclusion-zone entry points exist in the header, the binding and the library; the setting's structure and the table's layout
agree on both sides; the pipeline configuration carries the setting with defaults that mean "off"; optical_fusion hands it down
(CPU-only).  On a device: the setting's defaults, its round trip, every invalid field, and "off" after NULL."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_zones", "ofk_get_zones", "ofk_zones_step", "ofk_zones_reset", "ofk_zones_download")
FIELDS = ["mode", "link", "min_members", "radius", "ttl", "max_zones"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge


def test_entry_points_declared_bound_and_exported(built, ofk):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofk.h")).read(), flags=re.S)
    lib = ofk.load_library()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert s in ofk.SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
    for name, val in (("OFK_ZONES_OFF", 0), ("OFK_ZONES_HULL", 1), ("OFK_ZONE_MAX", 16), ("OFK_ZONE_VERTS", 32), ("OFK_ZONE_INTS", 67),
                      ("OFK_ZONE_FLOATS", 4), ("OFK_ZONE_STATS", 8)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
    assert (ofk.ZONES_OFF, ofk.ZONES_HULL, ofk.ZONE_MAX, ofk.ZONE_VERTS, ofk.ZONE_INTS, ofk.ZONE_FLOATS, ofk.ZONE_STATS) == (0, 1, 16, 32, 67, 4, 8)
    assert ofk.ZONE_INTS == 3 + 2 * ofk.ZONE_VERTS and ofk.ZONES_MODES == {"off": 0, "hull": 1}
    m = re.search(r"typedef struct ofk_zones \{(.*?)\} ofk_zones;", txt, flags=re.S)
    assert m and re.findall(r"\b(int|double)\s+(\w+);", m.group(1)) == [("int", n) for n in FIELDS]
    assert [(n, t) for n, t in ofk.Zones._fields_] == [(n, C.c_int) for n in FIELDS] and C.sizeof(ofk.Zones) == 24
    assert len(lib.ofk_zones_step.argtypes) == 12 and len(lib.ofk_zones_download.argtypes) == 4
    assert lib.ofk_set_zones(None, None) == ofk.E_INVALID and lib.ofk_get_zones(None, None) == ofk.E_INVALID
    assert lib.ofk_zones_reset(None, 1) == ofk.E_INVALID and lib.ofk_zones_download(None, None, None, None) == ofk.E_INVALID


def test_zone_kernels_are_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for k in (b"k_zones_update", b"k_zone_mask", b"k_zones_age", b"k_disc_mask"):
        assert k in blob, k


def test_settings_from_names(built, ofk):
    z = ofk.zones_setting()
    assert [getattr(z, n) for n in FIELDS] == [1, 48, 3, 20, 30, 16]
    z = ofk.zones_setting("hull", link=4096, min_members=1, radius=0, ttl=65535, max_zones=1)
    assert [getattr(z, n) for n in FIELDS] == [1, 4096, 1, 0, 65535, 1]
    assert ofk.zones_setting("off", link=0).mode == 0               # off: the other fields are not looked at
    for bad in (dict(mode="box"), dict(mode=2), dict(link=0), dict(link=4097), dict(min_members=0), dict(radius=-1), dict(radius=256), dict(ttl=0),
                dict(ttl=65536), dict(max_zones=0), dict(max_zones=17)):
        with pytest.raises(ValueError):
            ofk.zones_setting(**bad)
    with pytest.raises(TypeError):
        ofk.zones_setting(margin=3)


class Recorder:
    """Stands in for ofk.Context: records what a pipeline applies to it."""
    calls = []

    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        def f(*a, **k):
            Recorder.calls.append((name, a, k))
        return f


def test_pipeline_config_defaults_mean_off(built, pkg, ofk, monkeypatch):
    from of_amd import pipeline
    from of_amd.pipeline import PipelineConfig, FlowPipeline, FlowStream
    for cfg in (PipelineConfig(), PipelineConfig.node(), PipelineConfig.of_module(), PipelineConfig.evaluate_exp(), PipelineConfig.baseline_1080p()):
        assert (cfg.zones, cfg.zone_link, cfg.zone_min, cfg.zone_radius, cfg.zone_ttl, cfg.zone_max) == (None, 48, 3, 20, 30, 16)
        assert cfg.zones_setting() is None
    assert PipelineConfig(zones="off").zones_setting() is None
    on = PipelineConfig(zones="hull", zone_link=32, zone_min=4, zone_radius=12, zone_ttl=9, zone_max=5)
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params())          # to_params() does not know the setting
    assert [getattr(on.zones_setting(), n) for n in FIELDS] == [1, 32, 4, 12, 9, 5]
    assert [getattr(PipelineConfig(zones="hull").zones_setting(), n) for n in FIELDS] == [1, 48, 3, 20, 30, 16]
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    Recorder.calls = []
    s = FlowStream(64, 48, batch=1, cfg=PipelineConfig())
    FlowPipeline(64, 48, batch=1, cfg=on)                        # frame pairs ignore the setting
    assert not [c for c in Recorder.calls if c[0] == "set_zones"] and callable(s.zones)
    FlowStream(64, 48, batch=1, cfg=on)
    sets = [c for c in Recorder.calls if c[0] == "set_zones"]
    assert len(sets) == 1 and [getattr(sets[0][1][0], n) for n in FIELDS] == [1, 32, 4, 12, 9, 5]


def test_optical_fusion_hands_the_zone_setting_to_its_pipeline_config(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    from of_amd.velocity_node import optical_fusion
    assert optical_fusion(spin=False)._zones == {}
    node = optical_fusion(spin=False, zones=dict(link=40, radius=25, ttl=12))
    assert node._zones == dict(zones="hull", zone_link=40, zone_radius=25, zone_ttl=12)
    assert [getattr(PipelineConfig(**node._zones).zones_setting(), n) for n in FIELDS] == [1, 40, 3, 25, 12, 16]
    assert optical_fusion(spin=False, zones={})._zones == dict(zones="hull")
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, zones=dict(mode="box"))
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, zones=dict(margin=3))


@pytest.mark.gpu
def test_setting_round_trip_invalid_fields_and_off_after_null(pkg, ofk):
    ctx = ofk.Context(0, 64, 48, 2, 100, 2)
    try:
        assert [getattr(ctx.get_zones(), n) for n in FIELDS] == [0, 48, 3, 20, 30, 16]          # off, the defaults behind it
        ctx.set_zones(link=33, min_members=100, radius=255, ttl=65535, max_zones=7)
        assert [getattr(ctx.get_zones(), n) for n in FIELDS] == [1, 33, 100, 255, 65535, 7]
        good = dict(mode=1, link=33, min_members=100, radius=255, ttl=65535, max_zones=7)
        for bad in (dict(mode=2), dict(mode=-1), dict(link=0), dict(link=4097), dict(min_members=0), dict(min_members=101), dict(radius=-1),
                    dict(radius=256), dict(ttl=0), dict(ttl=65536), dict(max_zones=0), dict(max_zones=17)):
            with pytest.raises(ofk.OfkError) as e:
                ctx.set_zones(ofk.Zones(*[dict(good, **bad)[n] for n in FIELDS]))
            assert e.value.code == ofk.E_INVALID
            assert [getattr(ctx.get_zones(), n) for n in FIELDS] == [1, 33, 100, 255, 65535, 7], bad       # the previous setting is in place
        ctx.set_zones(None)
        assert ctx.get_zones().mode == 0
        ctx.set_zones(link=5)
        ctx.set_zones(ofk.Zones(0, -9, -9, -9, -9, -9))            # mode off: off, whatever else the structure holds
        assert ctx.get_zones().mode == 0 and ctx.get_zones().link == 5
        with pytest.raises(ofk.OfkError):                          # the stage entry needs the setting
            ctx.zones_step([[[1.0, 1.0]]], [[[1.0, 1.0]]], [[1]], [[0]], [1], 48, 64)
    finally:
        ctx.close()
