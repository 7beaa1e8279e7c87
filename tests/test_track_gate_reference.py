"""CPU-only: what the track gates buy, as conditions on the reference (tests/track_gate_reference.py): the rows of
lk_seed_reference.ROWS (640 x 480, 300 corners, window 15, 20 iterations, eps 0.03, plain forward LK with maxLevel 3) gated at
0.5 px.  "Wrong" = status 1 and more than 0.5 px from the true end point, over all corners; "good lost" = a right point dropped."""
import numpy as np
import pytest

import lk_seed_reference as R  # noqa: E402  (tests/lk_seed_reference.py)
import track_gate_reference as G  # noqa: E402  (tests/track_gate_reference.py)

_rows = {}


def row(name):
    if name not in _rows:
        _rows[name] = G.experiment_row(name)
    return _rows[name]


def test_table_of_every_row(pkg):
    print("\nrow          ungated tracked/wrong/rel   " + "   ".join(f"{l}: kept/wrong/good lost/rel" for l, _ in G.VARIANTS))
    for name in (r[0] for r in R.ROWS):
        t = row(name)
        u = t["ungated"]
        print(f"{name:12s} {u['kept']:3d}/{u['wrong']:3d}/{u['rel']:.4f}   " +
              "   ".join(f"{t[l]['kept']:3d}/{t[l]['wrong']:3d}/{t[l]['lost']:3d}/{t[l]['rel']:.4f}" for l, _ in G.VARIANTS))
        for l, _ in G.VARIANTS:                                  # a gate only ever removes points
            assert t[l]["kept"] <= u["kept"] and t[l]["kept"] + t[l]["lost"] + (u["wrong"] - t[l]["wrong"]) == u["kept"], (name, l)


def test_yaw_row_seeded_back_pass_removes_the_wrong_points(pkg):
    t = row("yaw0.15")
    u, g = t["ungated"], t["seeded L3"]
    assert u["wrong"] / u["kept"] >= 0.30, u                     # measured 0.407
    assert g["wrong"] / g["kept"] <= 0.10, g                     # measured 0.046
    assert g["lost"] <= 0.05 * g["good"], g                      # measured 2 of 169


def test_default_row_loses_no_good_points_and_reaches_the_solve_floor(pkg):
    t = row("default")
    u, g = t["ungated"], t["seeded L3"]
    assert g["lost"] <= 0.01 * g["good"], g
    assert u["rel"] >= 0.02, u                                   # measured 0.0260: one wrong point in 300
    assert g["rel"] <= 0.01, g                                   # measured 0.0064


def test_translation_row_is_beyond_the_gate(pkg):
    # The motion (60 px) is beyond what three pyramid levels reach.  The forward search ends in a wrong local minimum, and the backward
    # search, started in that minimum's neighbourhood, falls into the matching wrong minimum of the first frame, which lies within
    # 0.5 px of the original point: the few survivors come home and are wrong all the same.  Seeding the forward pass is the tool here.
    t = row("translation")
    u, g = t["ungated"], t["seeded L3"]
    assert g["kept"] < 0.10 * u["kept"], (g, u)                  # measured 23 of 288


def test_gate_off_is_the_plain_tracker(pkg):
    e = R.experiment_pair("yaw0.08")
    r = G.gated(e["g0"], e["g1"], e["pts"], max_level=3, gate=G.OFF, **R.EXP_LK)
    n, s, err = R.lk_pyr(e["g0"], e["g1"], e["pts"], max_level=3, **R.EXP_LK)
    assert np.array_equal(r["status"], s.ravel()) and np.array_equal(r["next"].view(np.uint32), n.reshape(-1, 2).view(np.uint32))
    assert np.array_equal(r["err"].view(np.uint32), err.ravel().view(np.uint32))
    assert list(r["stats"]) == [int(s.sum()), 0, 0, 0]


def test_err_cap_alone_and_levels(pkg):
    e = R.experiment_pair("yaw0.08")
    base = G.gated(e["g0"], e["g1"], e["pts"], max_level=3, gate=G.OFF, **R.EXP_LK)
    cap = float(np.median(base["err"][base["st_f"] == 1]))
    r = G.gated(e["g0"], e["g1"], e["pts"], max_level=3, gate=G.setting(err_max=cap), **R.EXP_LK)
    want = (base["st_f"] == 1) & (base["err"] <= np.float32(cap))
    assert np.array_equal(r["keep"], want) and r["stats"][3] == int((base["st_f"] == 1).sum() - want.sum()) and 0 < want.sum() < len(want)
    assert G.back_level(G.setting(fb="plain", fb_level=-1), 3) == 3 and G.back_level(G.setting(fb="plain", fb_level=5), 3) == 3
    assert G.back_level(G.setting(fb="seeded", fb_level=0), 3) == 0
