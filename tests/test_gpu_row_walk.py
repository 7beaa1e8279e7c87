"""The rows of a stream's per-track states stay in step: the same status gives the same layout in every state.

The track table, the depths, the keyframe, its map and the templates each compact their rows with the walk of csrc/k_rows.inc and
append fresh rows behind the kept ones.  Here the stage entries track_table_step, track_depth_step, keyframe_step,
keyframe_map_step and track_template_step get the same status, count, new count and max_total, and every state carries its row
index through the step in a field the step leaves alone (table: birth_xy; depths: rho, with nobs = 1, an unsolved step and update
off; keyframe: key_xy; map: key_rho; templates: A[0] under L = I).  Then, for every state,

    rows [0, kept)             hold the indices np.flatnonzero(status[:n]), in order,
    rows [kept, kept + extra)  hold the state's fresh values, extra = max(0, min(new count, max_total - kept, stride - kept)),
    rows [kept + extra, S)     are as they were.

Counts 0, 1, 64, 257 and 513 at a stride of 520, the "chunk-last" pattern (the last row of every chunk of 256 and row n - 1) and a
seeded random one; appended rows that fit, that max_total - kept cuts, and that stride - kept cuts.  The stage entries refuse
max_total > stride (ofk.h), so the last case runs at max_total == stride with more new rows than the stride has room for, and the
refusal itself is asserted.

A keyframe cannot hold on fewer than three rows (min_rows >= 3 is the setting's floor): with kept < 3 the step re-keys, which sets
key_xy to the next points - given here as the key points, so key_xy carries the index either way - and empties the map's key_rho
(rule M5), which is then what the kept rows must hold.  With kept >= 3 no entry re-keys, and that is asserted.

test_restatements_give_the_layout checks the same layout on the CPU restatements; test_device_gives_the_layout on the device."""
import zlib

import numpy as np
import pytest

import keyframe_map_reference as M
import keyframe_reference as K
import track_depth_reference as D
import track_table_reference as T
import track_template_reference as TP

S = 520
COUNTS = (0, 1, 64, 257, 513)
PATTERNS = ("chunk-last", "random")
APPENDS = ("fits", "budget", "stride")
STATES = ("table", "depth", "keyframe", "map", "template")
IDX = np.arange(S)
KEY_SET = K.setting(min_rows=3)
MAP_SET = M.setting()
DEPTH_SET = D.setting(update=0)
TPL_SET = TP.setting(scale_max=0.0)                              # never refreshed: det A is the row index here
STEP, NEXT_ID, IMG_H, IMG_W = 5, 9000, 48, 64


def make_case(n, pattern, kind):
    rng = np.random.default_rng(zlib.crc32(repr((n, pattern)).encode()))
    keep = (IDX % 256 == 255) | (IDX == n - 1) if pattern == "chunk-last" else rng.uniform(size=S) < 0.6
    status = (keep * rng.integers(1, 256, S)).astype(np.uint8)   # any non-zero byte keeps; rows beyond n are noise
    kept_rows = np.flatnonzero(status[:n])
    kept = len(kept_rows)
    new_count, max_total = {"fits": (7, S), "budget": (40, kept + 5), "stride": (S, S)}[kind]
    extra = max(0, min(new_count, max_total - kept, S - kept))   # the clamp, restated
    assert extra == {"fits": 7, "budget": 5, "stride": S - kept}[kind]
    new_pts = rng.uniform(0, 60, (S, 2)).astype(np.float32)
    key_xy = np.stack([IDX + 1.0, (IDX * 37) % 61 + 1.0], 1).astype(np.float32)
    sensors = np.zeros(28); sensors[0] = 1.0; sensors[3] = 1.0; sensors[[7, 11, 15]] = 1.0; sensors[19] = 1.0 / 500.0
    return dict(n=n, status=status, kept_rows=kept_rows, kept=kept, new_count=new_count, max_total=max_total, extra=extra, new_pts=new_pts,
                prev=rng.uniform(0, 60, (S, 2)).astype(np.float32), nxt=rng.uniform(0, 60, (S, 2)).astype(np.float32),
                x=rng.uniform(-0.1, 0.1, (S, 2)), u=rng.normal(0, 1e-3, (S, 2)), key_xy=key_xy, sensors=sensors, rekey=kept < 3,
                centre=np.tile(np.float32([IMG_W / 2, IMG_H / 2]), (S, 1)), img=np.zeros((IMG_H, IMG_W), np.uint8))


def table_in():
    t = T.empty(S)
    t["ids"][:] = IDX + 100; t["age"][:] = 1; t["birth_xy"][:] = np.stack([IDX + 1.0, IDX + 0.5], 1)
    t["step"], t["next_id"] = STEP, NEXT_ID
    return t


def depth_in():
    return dict(rho=IDX + 1.0, var=np.full(S, 0.25), nobs=np.ones(S, np.int32))


def key_in(c, with_map):
    st = (M if with_map else K).empty(S)
    st["key_xy"][:] = c["key_xy"]; st["member"][:] = 1; st["istate"][1] = 1     # a keyframe of key_step 0 with one member at the key
    if with_map:
        st["key_rho"][:] = IDX + 1.0; st["key_var"][:] = 0.01                   # mstate 0, 0: captured for key_step 0, no map rows
    return st


def template_in():
    st = TP.empty_state(S, TPL_SET.win)
    st["A"][:] = np.stack([IDX + 2.0, 0 * IDX, 0 * IDX, 1.0 + 0 * IDX], 1); st["ncc"][:] = 0.5; st["flag"][:] = 7; st["tstate"][:] = 1
    return st


def check_layout(c, rows, tag):
    """rows: per state (carried [S], what the kept rows must carry [kept], fresh [S] bool: the row holds the fresh values, before [S])."""
    kept, end = c["kept"], c["kept"] + c["extra"]
    assert set(rows) == set(STATES), tag
    for name, (carried, want, fresh, before) in rows.items():
        assert np.array_equal(carried[:kept], want), (tag, name, "kept rows", carried[:kept][:8], want[:8])
        assert fresh[kept:end].all(), (tag, name, "fresh rows", np.flatnonzero(~fresh[kept:end])[:8] + kept)
        assert np.array_equal(carried[end:], before[end:]) and not fresh[end:].any(), (tag, name, "rows behind the count")


def check_rekey(c, reasons, tag):
    for name, reason in reasons.items():
        assert (reason != 0) == c["rekey"], (tag, name, "re-key reason", reason)


def index_of(c, shift):
    return (c["kept_rows"] + shift).astype(np.float64)


def table_rows(c, t):
    j = np.arange(S) - c["kept"]
    with np.errstate(all="ignore"):
        born = c["new_pts"][np.clip(j, 0, S - 1)]
        fresh = ((t["ids"] == (NEXT_ID + j).astype(np.uint32)) & (t["age"] == 0) & (t["birth_step"] == STEP + 1) & (t["birth_xy"] == born).all(1) &
                 (t["flow_xy"] == 0).all(1))
    return t["birth_xy"][:, 0].astype(np.float64), index_of(c, 1), fresh, IDX + 1.0


def depth_rows(c, d):
    return d["rho"], index_of(c, 1), (d["rho"] == 0) & (d["var"] == 0) & (d["nobs"] == 0), IDX + 1.0


def key_rows(c, k):
    return k["key_xy"][:, 0].astype(np.float64), index_of(c, 1), (k["key_xy"] == 0).all(1) & (k["member"] == 0), IDX + 1.0


def map_rows(c, k):
    want = np.zeros(c["kept"]) if c["rekey"] else index_of(c, 1)       # rule M5: a re-key empties the key depths
    fresh = (k["key_rho"] == 0) & (k["key_var"] == 0)
    if c["rekey"]:
        fresh[:c["kept"]] = False                                # emptied, not appended
    return k["key_rho"], want, fresh, IDX + 1.0


def template_rows(c, t):
    fresh = (t["A"] == np.float32([1, 0, 0, 1])).all(1) & (t["ncc"] == 0) & (t["flag"] == 0) & (t["tstate"] == 0)
    return t["A"][:, 0].astype(np.float64), index_of(c, 2), fresh, IDX + 2.0


CASES = [(n, p) for n in COUNTS for p in PATTERNS]


@pytest.mark.parametrize("n,pattern", CASES)
def test_restatements_give_the_layout(n, pattern):
    for kind in APPENDS:
        c = make_case(n, pattern, kind)
        t = table_in(); t["count"] = n
        tab = T.update(t, c["prev"], c["nxt"], c["status"], c["new_pts"], c["new_count"], c["max_total"])[0]
        dep = D.step(depth_in(), c["x"], c["u"], c["status"], n, np.zeros(3), np.zeros(3), False, DEPTH_SET, c["new_count"], c["max_total"])[0]
        key, krec = K.step(key_in(c, False), c["key_xy"], c["status"], n, c["sensors"], np.zeros(3), True, STEP, KEY_SET, c["new_count"],
                           c["max_total"])[:2]
        kmap, mkrec = M.step(key_in(c, True), None, c["key_xy"], c["status"], n, c["sensors"], np.zeros(3), True, STEP, KEY_SET, MAP_SET,
                            c["new_count"], c["max_total"])[:2]
        _, st, tpl, _ = TP.template_step(c["img"], c["img"], c["centre"], c["centre"], c["status"], np.ones(S, np.int32), n, np.float32([1, 0, 0, 1]),
                                         template_in(), TPL_SET, c["new_count"], c["max_total"])
        tag = ("restatement", n, pattern, kind)
        assert tab["count"] == c["kept"] + c["extra"] and np.array_equal(st, c["status"]), tag
        check_rekey(c, dict(keyframe=int(krec[9]), map=int(mkrec[9])), tag)
        check_layout(c, dict(table=table_rows(c, tab), depth=depth_rows(c, dep), keyframe=key_rows(c, key), map=map_rows(c, kmap),
                             template=template_rows(c, tpl)), tag)


@pytest.fixture(scope="module")
def ctx(ofk):
    c = ofk.Context(0, 64, 48, 3, 1100, 2)
    yield c
    c.close()


def device_entries(ctx, ofk, c, max_total):
    """The five stage entries on the case's inputs, one stream each: per state a call that returns the entry's outputs."""
    n, st, nc = [c["n"]], c["status"][None], [c["new_count"]]
    batch = lambda d: {k: v[None] for k, v in d.items() if isinstance(v, np.ndarray)}
    d, s, m, p = DEPTH_SET, KEY_SET, MAP_SET, TPL_SET
    td = ofk.track_depth_setting(True, d["sigma_flow"], d["b_min"], d["gate"], d["q"], d["min_obs"], d["rel_max"], d["min_rows"], d["update"])
    kf = ofk.keyframe_setting(True, s["sigma_flow"], s["gate"], s["min_rows"], s["min_share"], s["rot_max"], s["max_age"])
    km = ofk.keyframe_map_setting(True, m["min_obs"], m["rel_max"], m["min_rows"], m["ready_share"], m["weights"])
    tp = ofk.track_template_setting(True, p.win, p.ncc_min, p.anchor_iters, p.anchor_max, "keep", p.fit_min, p.fit_gate, p.scale_max)
    key_args = (c["key_xy"][None], st, n, c["sensors"][None], np.zeros((1, 3)), [1], [STEP])
    return dict(
        table=lambda: ctx.track_table_step(batch(table_in()), [[STEP, NEXT_ID]], c["prev"][None], c["nxt"][None], st, n, c["new_pts"][None], nc, max_total, None),
        depth=lambda: ctx.track_depth_step(c["x"][None], c["u"][None], st, n, np.zeros((1, 3)), np.zeros((1, 3)), [0], batch(depth_in()), new_counts=nc,
                                           max_total=max_total, track_depth=td),
        keyframe=lambda: ctx.keyframe_step(*key_args, batch(key_in(c, False)), new_counts=nc, max_total=max_total, keyframe=kf),
        map=lambda: ctx.keyframe_map_step(*key_args, batch(key_in(c, True)), depth=None, new_counts=nc, max_total=max_total, keyframe=kf, keyframe_map=km),
        template=lambda: ctx.track_template_step(c["img"][None], c["img"][None], c["centre"][None], c["centre"][None], st, np.ones((1, S), np.int32), n,
                                                 np.float32([[1, 0, 0, 1]]), batch(template_in()), new_counts=nc, max_total=max_total, track_template=tp))


@pytest.mark.gpu
@pytest.mark.parametrize("n,pattern", CASES)
def test_device_gives_the_layout(ctx, ofk, n, pattern):
    for kind in APPENDS:
        c = make_case(n, pattern, kind)
        got = {name: call() for name, call in device_entries(ctx, ofk, c, c["max_total"]).items()}
        one = lambda d: {k: v[0] for k, v in d.items()}
        tab, dep, key, kmap, tpl = (one(got[name][i]) for name, i in (("table", 0), ("depth", 0), ("keyframe", 0), ("map", 0), ("template", 2)))
        tag = ("device", n, pattern, kind)
        assert got["table"][2][0] == c["kept"] + c["extra"] and np.array_equal(got["template"][1][0], c["status"]), tag
        check_rekey(c, dict(keyframe=int(got["keyframe"][1][0, 9]), map=int(got["map"][1][0, 9])), tag)
        check_layout(c, dict(table=table_rows(c, tab), depth=depth_rows(c, dep), keyframe=key_rows(c, key), map=map_rows(c, kmap),
                             template=template_rows(c, tpl)), tag)


@pytest.mark.gpu
def test_stage_entries_refuse_a_budget_beyond_the_stride(ctx, ofk):
    """max_total <= stride is the entries' contract: stride - kept is never the smaller clamp there."""
    c = make_case(64, "random", "fits")
    for name, call in device_entries(ctx, ofk, c, S + 1).items():
        with pytest.raises(ofk.OfkError, match="max_total"):
            call()
