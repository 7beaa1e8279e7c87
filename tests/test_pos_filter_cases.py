"""The case table of tests/test_gpu_pos_filter.py (a) is not vacuous (CPU-only, on the restatement): each of the three updates shows
every outcome at least once, clones occur on fresh steps and on steps that are not fresh, a broken input switches exactly its own
update off and leaves the state finite."""
import numpy as np

import pos_filter_cases as PC
import pos_filter_reference as R


def test_every_update_shows_every_outcome_and_clones_fall_on_fresh_and_other_steps():
    seen = {k: set() for k in range(3)}
    clones = set()
    for g in PC.groups():
        for sc, rows in zip(g["scripts"], PC.restate(g)):
            fresh = 1
            for (st, rec), s in zip(rows, sc["steps"]):
                for k in range(3):
                    seen[k].add(int(rec[25 + 5 * k]))
                if rec[40]:
                    clones.add((fresh, int(rec[30] != R.NOT)))
                fresh = int(rec[41])
                assert np.isfinite(st["x"]).all() and np.isfinite(st["P"]).all(), (g["name"], sc["name"])
    assert all(seen[k] == {R.NOT, R.APPLIED, R.GATED, R.REFUSED} for k in range(3)), seen
    assert {(1, 0), (1, 1), (0, 0), (0, 1)} <= clones, clones     # fresh or not on entry, with and without a displacement update


def test_the_combinations_are_the_ones_they_are_named_after():
    g = PC.groups()[0]
    rows = PC.restate(g)
    names = [sc["name"] for sc in g["scripts"]]
    for name, r in zip(names, rows):
        rec = r[-1][1]
        att = [int(rec[25 + 5 * k] != R.NOT) for k in range(3)]
        if name.startswith("fresh"):
            fresh, clone = int(name[5]), int(name[12])
            assert att == [int(name[15]), int(name[17]), int(name[19])], name
            assert r[0][1][41] == fresh and rec[40] == clone, name
        else:                                                    # a broken input: its own update is not attempted, the others are
            what = name.split("=")[0].split("<")[0].rstrip("012")
            want = dict(v=[0, 1, 1], D=[1, 0, 1], C_T=[1, 0, 1], rw=[1, 0, 1], fix=[1, 1, 0], sigma=[1, 1, 0], du=[1, 1, 1])[what]
            assert att == want, (name, att)
    assert len(names) == 32 + 24


def test_the_held_bias_group_holds_it_exactly():
    g = [x for x in PC.groups() if x["name"] == "held-bias"][0]
    for rows in PC.restate(g):
        for st, rec in rows:
            assert not st["P"][6:9].any() and not st["P"][:, 6:9].any() and not st["x"][6:9].any() and rec[24] == 0.0
