"""CPU-only: the restated track table (tests/track_table_reference.py) keeps its invariants over a random life of one stream, and the
ramp experiment meets its two conditions on the CPU reference tracker alone."""
import numpy as np
import pytest

import track_table_reference as T


def test_invariants_over_a_random_life():
    """30 steps with losses, appends clamped by max_total, one replace and one held step: ids unique, kept ids in order, age = steps
    survived, next_id = tracks ever born, step_ids = the ids before the step."""
    rng = np.random.default_rng(5)
    S, max_total = 96, 64
    pts = rng.uniform(0, 300, (S, 2)).astype(np.float32)
    t, stats = T.begin(pts, 60, S)
    assert list(stats) == [60, 0, 0, 60, 0, 0, 60, 0]
    born, survived, birth = 60, {i: 0 for i in range(60)}, {i: 0 for i in range(60)}
    clamped = 0
    for k in range(30):
        n = t["count"]
        ids_before = t["ids"][:n].copy()
        if k == 11:                                              # a replace in front of the step
            new = rng.uniform(0, 300, (S, 2)).astype(np.float32)
            t, st = T.replace(t, new, 35)
            assert list(st) == [35, 0, n, 35, 0, t["step"], born + 35, 0]
            assert np.array_equal(t["ids"][:35], np.arange(born, born + 35)) and np.array_equal(t["birth_xy"][:35], new[:35])
            for i in range(born, born + 35):
                survived[i], birth[i] = 0, t["step"]
            born += 35
            n, pts = 35, new
            ids_before = t["ids"][:n].copy()
        if k == 17:                                              # a held step: nothing is called, nothing changes
            held = T.copy(t)
            assert all(np.array_equal(held[key], t[key]) if isinstance(t[key], np.ndarray) else held[key] == t[key] for key in t)
            continue
        status = (rng.uniform(size=S) < 0.8).astype(np.uint8) * rng.integers(1, 3, S).astype(np.uint8)   # kept rows: 1 or 2, both non-zero
        nxt = (pts + rng.normal(0, 3, (S, 2))).astype(np.float32)
        n_new = int(rng.integers(0, 70)) if k % 3 == 0 else None
        new = rng.uniform(0, 300, (S, 2)).astype(np.float32)
        t2, step_ids, st = T.update(t, pts, nxt, status, new if n_new is not None else None, n_new, max_total, seed=True, gain=1.0)
        keep = np.flatnonzero(status[:n] != 0)
        kept, extra = len(keep), st[3]
        assert np.array_equal(step_ids, ids_before)
        assert np.array_equal(t2["ids"][:kept], ids_before[keep])                       # kept ids keep their relative order
        assert np.array_equal(t2["flow_xy"][:kept], nxt[keep] - pts[keep])
        assert extra == (0 if n_new is None else max(0, min(n_new, max_total - kept)))
        clamped += n_new is not None and n_new > max_total - kept
        assert np.array_equal(t2["ids"][kept:kept + extra], np.arange(born, born + extra))
        for i in ids_before[keep]:
            survived[int(i)] += 1
        for i in range(born, born + extra):
            survived[i], birth[i] = 0, t["step"] + 1
        born += extra
        c = t2["count"]
        assert c == kept + extra <= max(max_total, kept) and t2["step"] == t["step"] + 1 and t2["next_id"] == born
        assert len(set(t2["ids"][:c].tolist())) == c                                    # unique per stream
        assert [survived[int(i)] for i in t2["ids"][:c]] == t2["age"][:c].tolist()
        assert [birth[int(i)] for i in t2["ids"][:c]] == t2["birth_step"][:c].tolist()
        assert list(st[:3]) == [c, kept, n - kept] and st[4] == (t2["age"][:c].max() if c else 0) and list(st[5:7]) == [t2["step"], born]
        assert st[7] == np.count_nonzero(t["age"][:n] >= 1)                             # every finite flow seeds
        t = t2
        pts = np.concatenate([nxt[keep], new[:extra], np.zeros((S - c, 2), np.float32)])
    assert clamped >= 2 and t["step"] == 29


def test_seed_rule():
    pts = np.array([[10, 20], [30, 40], [5e5, 7], [50, 60], [70, 80]], np.float32)
    age = np.array([0, 2, 1, 1, 3], np.int32)
    flow = np.array([[9, 9], [1.5, -2.25], [1.2e6, 0], [np.nan, 1], [0.1, 0.2]], np.float32)
    model = pts + np.float32(100)
    got = T.seed_points(pts, 4, age, flow, 0.5, model)
    want = np.array([model[0], pts[1] + np.float32(0.5) * flow[1], pts[2], pts[3], model[4]], np.float32)     # row 4 is beyond the count
    assert np.array_equal(got, want)
    assert np.array_equal(T.seed_points(pts, 5, age, flow, 1.0)[[0, 2, 3]], pts[[0, 2, 3]])                    # age 0, beyond 1e6, NaN


@pytest.fixture(scope="module")
def tables():
    return {name: (T.run_experiment(name, 3, False), T.run_experiment(name, 1, True)) for name in T.EXP_ROWS}


def test_seeded_one_level_holds_every_step(tables):
    """Condition 1: seeded maxLevel 1 is good on at least SEEDED_MIN_GOOD of the inside corners at every step of every row."""
    for name, (_, seeded) in tables.items():
        print(name, "seeded maxLevel 1:", " ".join("%d/%d" % r for r in seeded))
        assert len(seeded) == 12 and all(i > 0 for _, i in seeded), name
        assert min(T.shares(seeded)) >= T.SEEDED_MIN_GOOD, (name, seeded)


def test_plain_four_levels_falls_behind(tables):
    """Condition 2: at the last step plain maxLevel 3's share lies at least PLAIN_GAP below the seeded maxLevel-1 share, every row."""
    for name, (plain, seeded) in tables.items():
        print(name, "plain maxLevel 3:", " ".join("%d/%d" % r for r in plain))
        assert T.shares(plain)[-1] <= T.shares(seeded)[-1] - T.PLAIN_GAP, (name, plain[-1], seeded[-1])
