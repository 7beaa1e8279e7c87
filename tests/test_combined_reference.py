"""CPU only: the composed reference (tests/combined_cases.py over stream_oracle.NodeLoop / oracle_of_module with their plugs and
batch_oracle.combined_chain) on the sequences tests/test_gpu_settings_combined.py runs on the device.  Every run must be active in
every setting it switches on - a comparison with the device means nothing where a setting never bit - and free of near-ties on every
step.  The counters are those of the committed code, written down here as test_zones_reference.py writes its figures down; the
wrong references the GPU tests' self-checks name (a gate-refused point counted as a reject; a table aged on a held step) are shown
to differ from the right ones in exactly what those tests assert."""
import numpy as np
import pytest

import combined_cases as cc

# zones inserted / refreshed, re-detections behind a live zone, points the gate refused with forward status 1, steps with such points
# AND rejects, points the solve stage dropped, re-detections where the grid examined more candidates than it accepted, NIS-gated steps
EXPECTED = {
    "all-fused": dict(inserted=2, refreshed=3, masked=14, refused=302, refused_with_rejects=8, dropped=53, grid_bound=12, nis_gated=4, cov_records=14),
    "all-step": dict(inserted=2, refreshed=3, masked=14, refused=159, refused_with_rejects=8, dropped=53, grid_bound=12, nis_gated=0, cov_records=14),
    "grid-zones": dict(inserted=3, refreshed=12, masked=14, refused=0, refused_with_rejects=0, dropped=139, grid_bound=11, nis_gated=0, cov_records=0),
    "gate-zones": dict(inserted=6, refreshed=0, masked=12, refused=194, refused_with_rejects=6, dropped=44, grid_bound=0, nis_gated=0, cov_records=0),
    "seed-gate-robust": dict(inserted=0, refreshed=0, masked=0, refused=191, refused_with_rejects=0, dropped=102, grid_bound=0, nis_gated=0, cov_records=0),
    "feasibility": dict(inserted=7, refreshed=10, masked=12, refused=0, refused_with_rejects=0, dropped=87, grid_bound=0, nis_gated=0, cov_records=0),
}


@pytest.fixture(scope="module")
def scene(pkg):
    from of_amd import synth, ofk
    frames, info = cc.sequences(synth)
    return frames, info, cc.sensor_rows(ofk, info)


def run(name, scene, **kw):
    from of_amd.pipeline import PipelineConfig
    frames, info, sr = scene
    ref = cc.Reference(name, PipelineConfig, frames, info, sr, **kw)
    steps = []
    for t in range(1, cc.NF):
        msgs = cc.imu_batch(t) if ref.kind == "ekf6" else [()] * cc.NB
        row = []
        for b in range(cc.NB):
            o = ref.step(t, b, msgs[b])                          # asserts gap >= 1e-6 and near == 0 where the robust solve runs
            if ref.cov_on:
                o["cov"] = ref.cov_record(b, o)[0]
            row.append(o)
        steps.append(row)
    return ref, steps


@pytest.mark.parametrize("name", list(cc.CASES))
def test_every_run_is_active_in_every_setting_it_switches_on(pkg, scene, name):
    ref, steps = run(name, scene)
    c = ref.counters
    print(name, c)
    assert c["solved"] == (cc.NF - 1) * cc.NB
    if ref.zones_on:
        assert c["inserted"] > 0 and c["masked"] > 0
    if ref.gated:
        assert c["refused"] > 0
        if ref.zones_on:
            assert c["refused_with_rejects"] > 0
    if ref.seeded:
        assert c["seeded"] == c["solved"]
    if ref.grid_on:
        assert c["grid_bound"] > 0 and c["examined"] > c["accepted"]
        assert all(st[0] == 192 and st[1] > st[0] for lg in ref.first_grid for st in lg)       # the first detection fills every cell
    if ref.robust_on or ref.cfg.use_feasibility:
        assert c["dropped"] > 0
    if ref.cov_on:
        assert c["cov_records"] == c["solved"] and all(o["cov"][13] == 0 for row in steps for o in row)
    if ref.filters is not None:
        assert 0 < c["nis_gated"] < c["nis_steps"] == c["solved"]
        nis = np.array([o["cov"][14] for row in steps for o in row])
        assert np.all(np.abs(nis / cc.NIS_MAX - 1) > 1e-3), nis                                # no NIS near the gate's threshold
    if name == "feasibility":
        assert not ref.robust_on and c["rejects"] == c["dropped"]                              # the feasibility rule alone feeds the zones
    assert {k: c[k] for k in EXPECTED[name]} == EXPECTED[name]


def test_gate_zones_tells_a_refused_point_from_a_reject(pkg, scene):
    """Rule 1 of the zones: "status behind the track gates".  The step test_gpu_settings_combined.py asserts stats[4] on is the first
    one, where both streams have gate-refused points with forward status 1 AND rejects; a reference that fed the zones the status ahead
    of the gates counts more rejects there, so the device's count cannot equal both."""
    ref, steps = run("gate-zones", scene)
    wrong, wsteps = run("gate-zones", scene, reject_status="forward")
    for b in range(cc.NB):
        o, q = steps[0][b], wsteps[0][b]
        assert o["refused"] > 0 and o["zones"].stats[4] > 0
        assert q["zones"].stats[4] > o["zones"].stats[4], (b, q["zones"].stats, o["zones"].stats)
        assert not np.array_equal(q["zones"].zones, o["zones"].zones)
    assert [int(steps[0][b]["zones"].stats[4]) for b in range(cc.NB)] == [10, 12]


def ofm(pkg):
    from of_amd import synth
    from of_amd.of_library import pix_trans
    from of_amd.pipeline import PipelineConfig, FusionConfig
    return cc.sequences(synth)[0], PipelineConfig, FusionConfig, pix_trans


def test_legacy_keep_feeds_the_zones_and_the_replacing_detection_runs_through_the_grid(pkg):
    frames, PipelineConfig, FusionConfig, pix_trans = ofm(pkg)
    cfg = cc.of_module_cfg(PipelineConfig)
    inp = cc.of_module_inputs(pix_trans)
    model = FusionConfig.of_module(synthetic_flow=False).model
    tot = dict(inserted=0, masked=0, rejects=0, bound=0, solved=0)
    for b in range(cc.NB):
        log = []
        first, steps = cc.of_module_reference(frames[b], cfg, inp, b, model, grid_log=log)
        for s in steps:
            z = s[6]
            tot["inserted"] += int(z["zones"].stats[1]); tot["rejects"] += z["rejects"]; tot["solved"] += int(s[0] is not None)
            tot["masked"] += int(z["redetected"] and z["zones_masked"] > 0)
        tot["bound"] += sum(int(ex > acc) for acc, ex in log[1:])
    print("of_module:", tot)
    assert tot == dict(inserted=10, masked=10, rejects=56, bound=10, solved=14)


def test_held_step_leaves_the_table_and_an_aged_one_differs(pkg):
    frames, PipelineConfig, FusionConfig, pix_trans = ofm(pkg)
    cfg = cc.of_module_cfg(PipelineConfig, grid=None)
    inp = cc.of_module_inputs(pix_trans, nb=1, held=True)
    model = FusionConfig.of_module(synthetic_flow=False, hold_on_skip=True).model
    first, steps = cc.of_module_reference(frames[1], cfg, inp, 0, model, hold=True)
    held = [t for t, s in enumerate(steps, 1) if s[6]["held"]]
    assert held == [cc.HELD_STEP] and all(s[0] is not None for t, s in enumerate(steps, 1) if t != cc.HELD_STEP)
    before, at = steps[cc.HELD_STEP - 2][6]["zones"], steps[cc.HELD_STEP - 1][6]["zones"]
    assert before.live() and np.array_equal(before.zones, at.zones) and np.array_equal(before.motion.view(np.uint32), at.motion.view(np.uint32))
    assert np.array_equal(before.stats, at.stats)
    assert sum(int(s[6]["zones"].stats[1]) for s in steps[cc.HELD_STEP:]) > 0                   # zones are inserted behind it too
    _, wrong = cc.of_module_reference(frames[1], cfg, inp, 0, model, hold=True, age_on_hold=True)
    aged = wrong[cc.HELD_STEP - 1][6]["zones"]
    assert not np.array_equal(aged.zones, at.zones) and not np.array_equal(aged.motion.view(np.uint32), at.motion.view(np.uint32))


PAIRS_EXPECTED = [(192, 20, 16), (192, 24, 19), (192, 26, 16)]  # corners, points the gate refused, tracked points of weight 0


def test_pair_chain_is_active_in_every_setting(pkg, scene):
    from of_amd import ofk
    from of_amd.pipeline import PipelineConfig
    frames, info = scene[0], scene[1]
    sr = cc.sensor_rows(ofk, info, len(cc.PAIR_FRAMES))
    cfg = PipelineConfig(**cc.PAIR_CFG)
    prev, nxt = cc.pair_frames(frames)
    refs = cc.pair_references(cfg, prev, nxt, sr)
    got = []
    for r in refs:
        tracked = r["status"] == 1
        got.append(dict(corners=len(r["pts"]), examined=int(r["grid_stats"][1]), refused=int(np.count_nonzero((r["gate"]["st_f"] == 1) & ~tracked)),
                        zero_weight=int(np.count_nonzero(tracked & (r["weights"] == 0))), cov_flag=float(r["cov"][13])))
        assert r["grid_stats"][1] > r["grid_stats"][0] and r["cov"][13] == 0 and r["rank"] == 3
    print("pairs:", got)
    assert all(g["refused"] > 0 and g["zero_weight"] > 0 for g in got)
    assert [(g["corners"], g["refused"], g["zero_weight"]) for g in got] == PAIRS_EXPECTED
