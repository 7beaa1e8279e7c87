"""The track-table entry points exist in the header, the binding and the library; the setting's structure agrees on both sides; the
kernels are in the code object; track_table_setting's defaults and every invalid field; the pipeline configuration and
optical_fusion carry the setting (CPU-only).  On a device: the setting's default, its round trip, every refusal leaving the setting
as it was, "off" after NULL, and the download's refusal before a run."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_track_table", "ofk_get_track_table", "ofk_track_table_download", "ofk_track_table_step", "ofk_track_seed_points")
FIELDS = ["mode", "seed", "gain"]


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
    for name, val in (("OFK_TT_OFF", 0), ("OFK_TT_ON", 1), ("OFK_TT_SEED_OFF", 0), ("OFK_TT_SEED_FLOW", 1), ("OFK_TT_STATS", 8)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
    assert (ofk.TT_OFF, ofk.TT_ON, ofk.TT_SEED_OFF, ofk.TT_SEED_FLOW, ofk.TT_STATS) == (0, 1, 0, 1, 8)
    assert ofk.TT_SEEDS == {"off": 0, "flow": 1}
    m = re.search(r"typedef struct ofk_track_table \{(.*?)\} ofk_track_table;", txt, flags=re.S)
    assert m and [n for _, n in re.findall(r"\b(int|double)\s+(\w+);", m.group(1))] == FIELDS
    assert [n for n, _ in ofk.TrackTable._fields_] == FIELDS
    assert [t for _, t in ofk.TrackTable._fields_] == [C.c_int, C.c_int, C.c_double]
    assert C.sizeof(ofk.TrackTable) == 16 and ofk.TrackTable.gain.offset == 8
    assert len(lib.ofk_track_table_download.argtypes) == 9 and len(lib.ofk_track_table_step.argtypes) == 19
    assert len(lib.ofk_track_seed_points.argtypes) == 10
    assert lib.ofk_set_track_table(None, None) == ofk.E_INVALID and lib.ofk_get_track_table(None, None) == ofk.E_INVALID
    assert lib.ofk_track_table_download(None, None, None, None, None, None, None, 1, None) == ofk.E_INVALID
    assert lib.ofk_track_table_step(None, None, *([None] * 12), 1, 1, 1, None, None) == ofk.E_INVALID
    assert lib.ofk_track_seed_points(None, None, None, 1, 1, None, None, 1.0, 0, None) == ofk.E_INVALID


def test_track_table_kernels_are_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    for k in (b"k_track_table_begin", b"k_track_table_replace", b"k_track_table_update", b"k_track_seed", b"k_update_tracks", b"k_seed_points"):
        assert k in blob, k


def test_settings_from_names(built, ofk):
    assert values(ofk.track_table_setting()) == [1, 0, 1.0]
    assert values(ofk.track_table_setting("flow")) == [1, 1, 1.0]
    assert values(ofk.track_table_setting("flow", 0.5)) == [1, 1, 0.5]
    assert values(ofk.track_table_setting(ofk.TT_SEED_FLOW, gain=-2.0)) == [1, 1, -2.0]
    assert values(ofk.track_table_setting(seed="off", gain=0.0)) == [1, 0, 0.0]
    assert ofk.track_table_setting(mode=ofk.TT_OFF, gain=float("nan")).mode == 0        # off: the gain is not looked at
    nan, inf = float("nan"), float("inf")
    for bad in (dict(seed="model"), dict(seed=2), dict(seed=-1), dict(gain=nan), dict(gain=inf), dict(gain=-inf), dict(mode=2), dict(mode=-1)):
        with pytest.raises(ValueError):
            ofk.track_table_setting(**bad)
    with pytest.raises(TypeError):
        ofk.track_table_setting(flow=True)


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
        assert cfg.track_table is None and cfg.track_table_setting() is None
    assert values(PipelineConfig(track_table=True).track_table_setting()) == [1, 0, 1.0]
    given = ofk.track_table_setting("flow", gain=0.75)
    on = PipelineConfig(track_table=given)
    assert values(on.track_table_setting()) == [1, 1, 0.75]
    assert bytes(on.to_params()) == bytes(PipelineConfig().to_params())          # to_params() does not know the setting
    assert PipelineConfig(track_table=ofk.track_table_setting(mode=ofk.TT_OFF)).track_table_setting() is None
    assert PipelineConfig(track_table=False).track_table_setting() is None
    with pytest.raises(ValueError):
        PipelineConfig(track_table=ofk.TrackTable(1, 2, 1.0)).track_table_setting()
    with pytest.raises(ValueError):
        PipelineConfig(track_table=ofk.TrackTable(1, 1, float("inf"))).track_table_setting()
    with pytest.raises(ValueError):
        PipelineConfig(track_table=ofk.TrackTable(7, 0, 1.0)).track_table_setting()
    with pytest.raises(ValueError):
        PipelineConfig(track_table="flow").track_table_setting()
    monkeypatch.setattr(pipeline.ofk, "Context", Recorder)
    Recorder.calls = []
    s = FlowStream(64, 48, batch=1, cfg=PipelineConfig())
    assert not [c for c in Recorder.calls if c[0] == "set_track_table"] and callable(s.track_table)
    FlowStream(64, 48, batch=1, cfg=on)
    FlowPipeline(64, 48, batch=1, cfg=on)                                         # independent pairs have no tracks: not applied
    sets = [c for c in Recorder.calls if c[0] == "set_track_table"]
    assert len(sets) == 1 and values(sets[0][1][0]) == [1, 1, 0.75]


def test_optical_fusion_hands_the_setting_to_its_pipeline_config(built, pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    from of_amd.velocity_node import optical_fusion
    assert optical_fusion(spin=False)._track_table == {}
    assert optical_fusion(spin=False, track_table=False)._track_table == {}
    node = optical_fusion(spin=False, track_table=True)
    assert values(PipelineConfig(**node._track_table).track_table_setting()) == [1, 0, 1.0]
    node = optical_fusion(spin=False, track_table=dict(seed="flow", gain=0.5))
    assert values(PipelineConfig(**node._track_table).track_table_setting()) == [1, 1, 0.5]
    given = ofk.track_table_setting("flow")
    assert optical_fusion(spin=False, track_table=given)._track_table["track_table"] is given
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, track_table=dict(seed="model"))
    with pytest.raises((TypeError, ValueError)):
        optical_fusion(spin=False, track_table=dict(flow=3))


@pytest.mark.gpu
def test_setting_round_trip_every_refusal_and_off_after_null(pkg, ofk):
    ctx = ofk.Context(0, 64, 48, 2, 100, 2)
    try:
        assert values(ctx.get_track_table()) == [0, 0, 1.0]        # off
        with pytest.raises(ofk.OfkError) as e:                     # no stream has run with the setting on yet
            ctx.track_table_download(1)
        assert e.value.code == ofk.E_INVALID
        ctx.set_track_table(ofk.TrackTable(1, 1, 0.25))
        assert values(ctx.get_track_table()) == [1, 1, 0.25]
        with pytest.raises(ofk.OfkError) as e:                     # the setting alone is no run
            ctx.track_table_download(1)
        assert e.value.code == ofk.E_INVALID
        nan, inf = float("nan"), float("inf")
        pts = np.zeros((1, 4, 2), np.float32)
        table = dict(ids=np.zeros((1, 4), np.uint32), age=np.zeros((1, 4), np.int32), birth_step=np.zeros((1, 4), np.int32), birth_xy=pts, flow_xy=pts)
        step = lambda m: ctx.track_table_step(table, np.zeros((1, 2), np.int32), pts, pts, np.ones((1, 4), np.uint8), [4], track_table=m)
        for bad in ((2, 1, 0.25), (-1, 1, 0.25), (1, 2, 0.25), (1, -1, 0.25), (1, 1, nan), (1, 1, inf), (1, 0, -inf)):
            for call in (ctx.set_track_table, step):
                with pytest.raises(ofk.OfkError) as e:
                    call(ofk.TrackTable(*bad))
                assert e.value.code == ofk.E_INVALID, bad
            assert values(ctx.get_track_table()) == [1, 1, 0.25], bad                    # the previous setting is in place
        for bad_gain in (nan, inf, -inf):
            with pytest.raises(ofk.OfkError):
                ctx.track_seed_points(pts, [4], np.ones((1, 4), np.int32), pts, gain=bad_gain)
        assert step(ofk.TrackTable(1, 1, 2.0))[4].shape == (1, 8)
        assert values(ctx.get_track_table()) == [1, 1, 0.25]       # the stage entries touch no setting
        ctx.set_track_table(None)
        assert values(ctx.get_track_table()) == [0, 1, 0.25]
        ctx.set_track_table(seed="flow", gain=0.5)
        ctx.set_track_table(ofk.TrackTable(0, 7, nan))             # mode off: off, whatever else it holds
        assert values(ctx.get_track_table()) == [0, 1, 0.5]
        with pytest.raises(ofk.OfkError):
            ctx.track_table_download(1)
    finally:
        ctx.close()
