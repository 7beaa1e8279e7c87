"""GPU: the per-track state of a stream with every track setting on at once, past 512 rows per stream (tests/track_state_cases.py).

The track table seeds LK with each track's flow, the seeded forward-backward gate and an err cap refuse rows, the templates drop and
re-anchor rows, the depths, the keyframe and its rotation keep a state per row - and every step compacts all of it, one kernel behind
the other, in passes of 256 rows.  Each test is one run of 7 steps over two streams of 240 x 320 (point_count_cases.stream_frames):

ladder        ofk_stream_step.  The streams begin with 256 corners; steps 1-4 land stream 0 on 257, 512, 513 and 600 tracks (so n_old
              is 256, 257, 512 and 513 in turn), steps 5-7 run at (600, 590).
twice         the ladder's calls on two fresh contexts: every row in use of every download has the same bits.  No atomics are used, so
              a race in an in-place compaction would show here.
fused-robust  ofk_stream_step_fused with the robust solve dropping rows behind the templates and the exclusion zones on, (600, 590); a
              textured rectangle moves over the ground (track_state_cases.frames_and_sensors says why).
replace       ofk_stream_step_fused with redetect_replace, (600, 520): some steps replace a stream's tracks, some do not.
zero          stream 1 loses its texture for two frames: all its rows are lost, steps run on 0 rows, then it refills to 600 beside
              a stream that keeps 500+ rows in the same launches.
hold          one stream with hold_on_skip; steps 3 and 4 go unsolved through min_solve and are held, at 600 rows.
switch        the templates on from step 2, the depths from 3, the keyframe from 4, its rotation from 5; the depths off at 5 and
              on again at 6, where they restart empty while the others live on.

After every call the composed follower compares the table (bit for bit), the depths (rho, var, nobs bit for bit, the record by
test_gpu_track_depth.same_record), the templates (track_template_reference.template_step in numpy: next, status, A, ncc, flag, tstate
and the template bytes bit for bit; the step map within 1e-10) and the keyframe with its rotation (key_xy and member bit for bit,
the records by the keyframe tests' same_record / same_rrec), and the id ledger checks every track by its id.  No row, stream or step is
exempt.  Every run ends with assertions on the device's own records that it did not pass idle; WAIVED names, per run, the ones its plan
cannot meet, and why.  The largest deviations met are printed (-s)."""
import numpy as np
import pytest

import point_count_cases as P
import track_state_cases as C

pytestmark = pytest.mark.gpu
LADDER = (257, 512, 513, 600)
PLANS = {"ladder": (600, 590), "fused-robust": (600, 590), "replace": (600, 520), "zero": (600, 590), "hold": (600, 590), "switch": (600, 590)}
SWITCH = {2: [("template", True)], 3: [("depth", True)], 4: [("key", True)], 5: [("rot", True), ("depth", False)], 6: [("depth", True)]}
# what a run's plan cannot meet:
WAIVED = {
    "ladder": {"solve_drops"},                                   # a plain step: nothing drops rows behind the templates
    "fused-robust": set(),
    "replace": {"straddled", "solve_drops", "map_solves"},       # a replace run appends nothing behind the solve, and from step 3 on every stream starts over
                                                                 # at every step (it is given max_corners - count corners, fewer than 520): no row matures
    "zero": {"solve_drops"},
    "hold": {"solve_drops"},
    "switch": {"solve_drops", "map_solves"},                     # the depths never live three steps in a row: no row matures
}
_asked = {}


def run(ofk, kind, follow=True, asked=None):
    """One run.  follow: with the composed follower and the ledgers (else: the calls alone, from `asked`).  -> (what every call
    returned and every download behind it, asked [t] = (max_corners, min_features), the follower)."""
    from of_amd.pipeline import FusionConfig
    nb = 1 if kind == "hold" else C.B
    fused = kind in ("fused-robust", "replace", "hold")
    robust = kind == "fused-robust"
    frames, sensors = C.frames_and_sensors(kind == "zero", nb, moving=robust)
    cfg = P.stream_cfg(600, "robust-fused" if robust else None, True)
    fusion = FusionConfig(use_imu=False, redetect_replace=kind == "replace", hold_on_skip=kind == "hold") if fused else None
    on = set() if kind == "switch" else set(C.ALL_ON)
    mc0, mf0 = PLANS[kind]
    ctx = C.open_context(ofk, nb, cfg, on=[n for n in C.ALL_ON if n in on], robust=robust, zones=robust, fused=fused)
    stage = ofk.Context(0, C.W, C.H, nb, C.S, cfg.max_level) if follow else None
    out, said, fol = [], [], None
    try:
        tracks, counts = ctx.stream_begin(frames[:, 0], C.step_cfg(cfg, 256 if kind == "ladder" else mc0).to_params())
        out.append((tracks.copy(), counts.copy(), ctx.track_table_download(nb, C.S)))
        if kind == "ladder":
            assert list(counts) == [256] * nb, counts
        if follow:
            fol = C.Follower(ofk, ctx, stage, cfg, sensors, tracks, counts, on=[n for n in C.ALL_ON if n in on], fused=fused, solve_drops=robust)
        for t in range(1, C.NF):
            for name, state in SWITCH.get(t, []) if kind == "switch" else []:
                C.switch(ctx, ofk, name, state)
                (on.add if state else on.discard)(name)
                if fol:
                    (fol.start if state else fol.stop)(name)
            mc, mf, land = mc0, mf0, None
            if fol:
                fol.look(frames[:, t], replace=(mf, mc) if kind == "replace" else None)
            if kind == "ladder" and t <= len(LADDER):
                land = LADDER[t - 1]
                mc, mf = C.landing(land, fol.c[0].n, fol.will_keep(0)) if fol else asked[t - 1]
            said.append((mc, mf))
            params = C.step_cfg(cfg, mc).to_params()
            if fused:
                fs = fusion.to_struct()
                if kind == "hold" and t in (3, 4):
                    fs.min_solve = 10 ** 6                       # more points than there are: not solved
                rec, fz, tracks, counts = ctx.stream_step_fused(frames[:, t], sensors, params, fs, mf, P.MASK_RADIUS)
            else:
                rec, tracks, counts = ctx.stream_step(frames[:, t], sensors, params, mf, P.MASK_RADIUS)
                fz = np.zeros(0)
            assert counts.max() <= mc, (kind, t, "a stream holds more tracks than the step returns", counts, mc)
            hold = kind == "hold" and rec[0, 15] == 0
            assert hold == (kind == "hold" and t in (3, 4)), (kind, t, rec[0, 15])
            d = fol.step(rec, tracks, counts, mc, (kind, t), held=hold) if fol else C.downloads(ctx, nb, on)
            out.append((rec.copy(), fz.copy(), tracks.copy(), counts.copy(), d))
            if fol:
                print(kind, "step", t, "asked", (mc, mf), "n_old", fol.ahead["n_old"], "->", [int(c) for c in counts], "held" if hold else "",
                      "solve: rows used, tracked %s" % rec[:, [11, 13]].tolist() if fused else "", "dropped by the solve so far", fol.seen["solve_drops"])
                lk, n0 = fol.ahead["lk"], fol.ahead["n_old"][0]
                err = lk["err"][0, :n0][lk["status"][0, :n0] != 0]
                if len(err):
                    print("    stream 0: LK err of the rows behind the gates, 50 / 90 / 99 %:", np.percentile(err, [50, 90, 99]).round(2),
                          "gate stats", fol.ctx.track_gate_stats(nb).tolist())
                if "template" in on and counts[0] and not hold:
                    p = d["template"]
                    A = p["A"][0, :counts[0]].astype(np.float64)
                    print("    template records 10-19", p["rec"][:, 10:20].astype(int).tolist(), "ncc 1 / 5 / 50 %:",
                          np.percentile(p["ncc"][0, :counts[0]][p["flag"][0, :counts[0]] & 15 == 1], [1, 5, 50]).round(4) if (p["flag"][0, :counts[0]] & 15 == 1).any() else None,
                          "det A max", (A[:, 0] * A[:, 3] - A[:, 1] * A[:, 2]).max().round(5))
                if "key" in on:
                    print("    keyframe flag, reason, live", d["key"]["rec"][:, [3, 9, 28]].tolist(), "rotation flag", d["rot"]["rec"][:, 3].tolist() if "rot" in on else None,
                          "depth flag, mature, updated, initialised", d["depth"]["rec"][:, [3, 4, 5, 6]].tolist() if "depth" in on else None)
            if land is not None:
                assert counts[0] == land, (kind, t, "stream 0 did not land", counts, land, mc)
    finally:
        ctx.close()
        if stage is not None:
            stage.close()
    return out, said, fol


def active(kind, fol):
    """The run did not pass idle: the conditions of the module's docstring, on the device's own records."""
    seen = dict(fol.seen)
    seen["moved_256"] = sum(l.moved_down[256] for l in fol.ledger); seen["moved_512"] = sum(l.moved_down[512] for l in fol.ledger)
    seen["straddled"] = sum(l.straddled[512] for l in fol.ledger)
    seen["big"] = sum(n > 512 for n in seen.pop("n_old"))
    print(kind, "activity:", seen)
    print(kind, "largest deviations so far, in units of their groups' scale:", C.DEV)
    need = dict(big=4, refused=1, template_drops=1, refreshed=1, solve_drops=1, moved_256=1, moved_512=1, straddled=1, rekeys_later=1, map_solves=1)
    for name, least in need.items():
        if name not in WAIVED[kind]:
            assert seen[name] >= least, (kind, name, seen)
    return seen


def test_ladder(pkg, ofk):
    out, said, fol = run(ofk, "ladder")
    _asked["ladder"] = said
    active("ladder", fol)
    n_old = [n for n in fol.seen["n_old"][0::C.B]]              # stream 0
    assert n_old[:4] == [256, 257, 512, 513] and said[4:] == [(600, 590)] * 3, (n_old, said)


def same(a, b, tag):
    if isinstance(a, dict):
        for k in a:
            same(a[k], b[k], tag + (k,))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), tag
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, tag + (i,))
    else:
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), tag


def rows_in_use(out):
    """A run's returns and downloads cut to the rows in use.  What lies behind a stream's count - in the returned tracks, in every
    per-row download, in the padding of a template's bytes and in the bytes of a row that has no template - is whatever the
    device's memory held when the context was made, and differs from context to context."""
    res, n_old = [], [int(c) for c in out[0][1]]
    tracks, counts, table = out[0]
    res.append(([tracks[b, :counts[b]] for b in range(len(counts))], counts, [{k: table[k][b, :counts[b]] for k in C.GT.KEYS} for b in range(len(counts))], table["stats"]))
    e2 = C.e2_of()
    for rec, fz, tracks, counts, d in out[1:]:
        per = []
        for b, c in enumerate(int(c) for c in counts):
            row = dict(tracks=tracks[b, :c], step_ids=d["table"]["step_ids"][b, :n_old[b]], next=d["last"]["next"][b, :n_old[b]], keep=d["last"]["keep"][b, :n_old[b]])
            row.update({k: d["table"][k][b, :c] for k in C.GT.KEYS})
            row.update({k: d["depth"][k][b, :c] for k in C.GD.KEYS})
            row.update({k: d["template"][k][b, :c] for k in ("A", "ncc", "flag", "tstate")})
            row["tmpl"] = d["template"]["tmpl"][b, :c, :e2][d["template"]["tstate"][b, :c] != 0]
            row.update(key_xy=d["key"]["key_xy"][b, :c], member=d["key"]["member"][b, :c])
            per.append(row)
        res.append((rec, fz, counts, per, d["table"]["stats"], d["depth"]["rec"], d["template"]["rec"], d["key"]["rec"], d["key"]["R_acc"], d["rot"]["rec"]))
        n_old = [int(c) for c in counts]
    return res


def test_twice(pkg, ofk):
    if "ladder" not in _asked:
        _asked["ladder"] = run(ofk, "ladder")[1]
    a, said_a, _ = run(ofk, "ladder", follow=False, asked=_asked["ladder"])
    b, said_b, _ = run(ofk, "ladder", follow=False, asked=_asked["ladder"])
    assert said_a == said_b == _asked["ladder"]
    assert [int(o[3][0]) for o in a[1:5]] == list(LADDER)
    same(rows_in_use(a), rows_in_use(b), ("twice",))


def test_fused_robust(pkg, ofk):
    _, _, fol = run(ofk, "fused-robust")
    active("fused-robust", fol)


def test_replace(pkg, ofk):
    _, _, fol = run(ofk, "replace")
    seen = active("replace", fol)
    assert 1 <= seen["replaced"] < len(fol.seen["n_old"]), seen  # some steps replace and some do not


def test_zero(pkg, ofk):
    out, _, fol = run(ofk, "zero")
    seen = active("zero", fol)
    n1 = fol.seen["n_old"][1::C.B]                               # the stream that loses its texture
    assert seen["zero_rows"] >= 1 and 0 in n1 and n1[n1.index(0):].count(600) >= 1 and min(fol.seen["n_old"][0::C.B]) > 500, (n1, out[-1][3])


def test_hold(pkg, ofk):
    _, _, fol = run(ofk, "hold")
    seen = active("hold", fol)
    assert seen["held"] == 2 and min(fol.seen["n_old"][2:4]) > 512, seen                       # the held steps ran past two chunks


def test_switch(pkg, ofk):
    _, _, fol = run(ofk, "switch")
    active("switch", fol)
