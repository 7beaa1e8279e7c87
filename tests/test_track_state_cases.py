"""CPU: the composed follower and the id ledger of tests/track_state_cases.py alone, with no GPU.

The table, depth, template and keyframe restatements run together (track_state_cases.Composed) over 600 rows in a stride of 640 on
synthetic status patterns: keep all, keep none, random, the first row of each 256-chunk only, the last row of each chunk only, and
appends past max_total.  The ledger accepts every one of these row-order restatements, and it rejects each of three deliberately
wrong compositions, each one a disagreement between two of a stream step's compactions that no record shows:

  depth-early       the depths compacted with the status in front of the templates' drop;
  template-noclamp  the templates' rows appended with max_total - kept but without the stride - kept clamp, so that the rows past one
                    stream's stride land on the first rows of the next stream;
  key-late          the keyframe's rows compacted one chunk late: chunk 2 written at the base of chunk 1.

The ledger's own rules are held to as well: a used id handed out again, a gap in the ids, a birth that moves, a held step that ages a
track, a replaced stream whose rows keep an old id or an old depth."""
import copy

import numpy as np
import pytest

import track_state_cases as C
import track_template_reference as TP
import keyframe_reference as K

F = np.float32
N, S_CPU = 600, 640
HI, WI = 120, 160
PATTERNS = ("all", "none", "random", "chunk-first", "chunk-last", "past-max-total")
KEY = K.setting(rot_max=0.5, min_share=0.0, min_rows=1)        # no re-key while a member lives: the key points have to be carried
TEMPLATE = TP.setting(outside=TP.DROP, anchor_iters=3, ncc_min=0.9, scale_max=1.2)
SHIFT = np.array([2, 1], F)                                      # the content moves by this much per frame
_cache = {}


def images():
    """Three frames cut from one texture, the content moving by SHIFT from one to the next."""
    if "img" not in _cache:
        tex = C.P.synth().make_texture(HI + 16, WI + 16, 21)
        tex = np.clip(np.rint(tex), 0, 255).astype(np.uint8)
        _cache["img"] = [tex[8 - k:8 - k + HI, 8 - 2 * k:8 - 2 * k + WI].copy() for k in range(3)]
    return _cache["img"]


def sensor_row():
    sn = np.zeros(28)
    sn[0] = 1.0; sn[3] = 1.0; sn[7:16] = np.eye(3).ravel(); sn[19] = 1.0 / 160; sn[20] = WI / 2; sn[21] = HI / 2
    return sn


V = np.array([0.0125, 0.00625, 0.0])                             # SHIFT in the sensors' units at depth 1


def status_of(pattern, rng):
    i = np.arange(S_CPU)
    st = {"all": np.ones(S_CPU, bool), "none": np.zeros(S_CPU, bool), "random": rng.uniform(size=S_CPU) < 0.6,
          "chunk-last": (i % 256 == 255) | (i == N - 1), "chunk-first": i % 256 == 0, "past-max-total": rng.uniform(size=S_CPU) < 0.8}[pattern]
    return (st * rng.integers(1, 256, S_CPU)).astype(np.uint8)  # any non-zero byte keeps; rows beyond the count are noise


def tracked(c, rng, wrong=0.0):
    """LK's next points of the rows of c: the content's shift and a little noise; a share `wrong` of them 3 px off (the templates
    drop those)."""
    n = c.n
    nxt = np.zeros((c.S, 2), F)
    nxt[:n] = c.pos + SHIFT + rng.uniform(-0.3, 0.3, (n, 2)).astype(F)
    off = rng.uniform(size=n) < wrong
    nxt[:n][off] += F(3)
    return nxt


def one_step(c, ledger, frame, lk_status, rng, new_count, max_total, wrong=0.0, replaced=False, **kw):
    """One step of Composed on frames (frame, frame + 1) -> (its snapshot for the ledger, what went in).  max_total None: five rows
    more than the templates keep, so that the budget cuts the append."""
    g0, g1 = images()[frame], images()[frame + 1]
    n_old, prev = c.n, c.padded(c.pos, F, 2)
    lk_next = tracked(c, rng, wrong)
    _, L = TP.affine_fit(prev, lk_next, lk_status, n_old, HI, WI, TEMPLATE)
    st = c.templates(g0, g1, lk_next, lk_status, L)[1]
    kept = int(np.count_nonzero(st[:n_old]))
    max_total = kept + 5 if max_total is None else max_total
    extra = max(0, min(new_count, max_total - kept))
    new_pts = np.column_stack([rng.uniform(12, WI - 15, extra), rng.uniform(12, HI - 14, extra)]).astype(F)
    nxt, keep = c.step(lk_next, lk_status, None, new_pts, max_total, sensor_row(), V, V, True, g0=g0, g1=g1, L=L, **kw)
    snap = c.snapshot(prev, nxt, keep, n_old, replaced=replaced)
    return snap, dict(prev=prev, lk_next=lk_next, lk_status=lk_status, keep=keep, nxt=nxt, kept=kept, n_old=n_old)


def base():
    """Composed and its ledger behind a first step that tracked all 600 rows: every row has a template, a key point and a depth.  The
    depths are then put into the middle of their lives (observation counts 0 .. 30), so that a row shifted onto its neighbour shows."""
    if "base" not in _cache:
        rng = np.random.default_rng(5)
        pts = np.column_stack([rng.uniform(12, WI - 15, N), rng.uniform(12, HI - 14, N)]).astype(F)
        c = C.Composed(S_CPU, pts, template=TEMPLATE, key=KEY, on=("template", "depth", "key"))
        ledger = C.Ledger("cpu")
        ledger.begin(c.table["ids"][:N], pts)
        snap, _ = one_step(c, ledger, 0, np.ones(S_CPU, np.uint8), rng, 0, S_CPU)
        ledger.step(snap, "step 1")
        assert c.n == N and c.trec[16] == N and c.krec[3] == K.NONE and c.drec[6] > 0.9 * N, (c.n, c.trec[10:20], c.krec[:10], c.drec[:10])
        c.depth["nobs"][:N] = rng.integers(0, 31, N)
        c.depth["rho"][:N] = np.where(c.depth["nobs"][:N] > 0, rng.uniform(0.8, 1.2, N), 0.0)
        c.depth["var"][:N] = np.where(c.depth["nobs"][:N] > 0, 0.01, 0.0)
        for i, q in zip(ledger.order, range(N)):
            ledger.rows[i]["nobs"] = int(c.depth["nobs"][q])
        _cache["base"] = (c, ledger)
    c, ledger = _cache["base"]
    return copy.deepcopy(c), copy.deepcopy(ledger)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_ledger_accepts_the_composed_restatements(pattern):
    """Step 2 under the pattern, step 3 on random flags: what step 2 moved across a chunk edge is read again."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(pattern.encode()))
    c, ledger = base()
    clamped = pattern == "past-max-total"
    snap, info = one_step(c, ledger, 1, status_of(pattern, rng), rng, 40 if clamped else 17, None if clamped else S_CPU, wrong=0.05)
    ledger.step(snap, (pattern, "step 2"))
    kept = info["kept"]
    if clamped:
        assert c.n == kept + 5 and c.stats[3] == 5, (c.n, kept, c.stats)                          # the budget cut the append
    if pattern == "all":
        assert c.trec[11] > 5 and kept < N and c.krec[9] == 0, (c.trec[10:20], c.krec[:10])        # templates dropped rows; no re-key
        assert ledger.moved_down[256] > 0 and ledger.moved_down[512] > 0, ledger.moved_down
    if pattern == "none":
        assert kept == 0 and c.n == 17
    if pattern in ("chunk-first", "chunk-last"):
        assert kept <= 4 and ledger.moved_down[512] >= 1, (kept, ledger.moved_down)
    st3 = np.zeros(S_CPU, np.uint8); st3[:c.n] = rng.uniform(size=c.n) < 0.7
    snap, _ = one_step(c, ledger, 0, st3, rng, 9, S_CPU, wrong=0.05)                               # the frames 0 -> 1 move by SHIFT as well
    ledger.step(snap, (pattern, "step 3"))


def test_ledger_rejects_depths_compacted_in_front_of_the_templates_drop():
    rng = np.random.default_rng(21)
    c, ledger = base()
    lk_status = status_of("all", rng)
    snap, info = one_step(c, ledger, 1, lk_status, rng, 17, S_CPU, wrong=0.05, depth_keep=lk_status)
    assert info["kept"] < info["n_old"]                          # the templates dropped rows the gates had let through
    with pytest.raises(C.LedgerError, match="observation count"):
        ledger.step(snap, "depth-early")
    c, ledger = base()                                           # the same step composed rightly passes
    rng = np.random.default_rng(21)
    snap, _ = one_step(c, ledger, 1, status_of("all", rng), rng, 17, S_CPU, wrong=0.05)
    ledger.step(snap, "depth as everything else")


def test_ledger_rejects_templates_appended_without_the_stride_clamp():
    """Two streams in one buffer of 2 x 640 rows.  Stream 0 keeps most of its 600 rows and is given 100 new corners at max_total
    700: min(100, max_total - kept) rows written from row `kept` on run past the stride into stream 1's first rows."""
    rng = np.random.default_rng(22)
    c0, _ = base()
    c1, ledger1 = base()
    _, info0 = one_step(c0, None, 1, status_of("all", rng), rng, 0, S_CPU, wrong=0.05)
    snap1, _ = one_step(c1, ledger1, 1, status_of("random", rng), rng, 17, S_CPU, wrong=0.05)
    over = min(100, 700 - info0["kept"]) - (S_CPU - info0["kept"])
    assert over > 0
    good = copy.deepcopy(ledger1)
    good.step(snap1, "stream 1 alone")
    t = {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in snap1["template"].items()}
    assert np.count_nonzero(t["tstate"][:over]) > over // 2      # there is something to lose
    t["tstate"][:over] = 0; t["flag"][:over] = 0
    with pytest.raises(C.LedgerError, match="refresh count"):
        ledger1.step(dict(snap1, template=t), "template-noclamp")


def test_ledger_rejects_keyframe_rows_compacted_one_chunk_late():
    rng = np.random.default_rng(23)
    c, ledger = base()
    before = {k: c.key[k].copy() for k in ("key_xy", "member")}
    snap, info = one_step(c, ledger, 1, status_of("random", rng), rng, 17, S_CPU, wrong=0.05)
    assert c.krec[9] == 0 and info["n_old"] > 512                # no re-key: the key points were carried; three chunks
    keep = info["keep"][:info["n_old"]] != 0
    per_chunk = [np.flatnonzero(keep[lo:lo + 256]) + lo for lo in (0, 256, 512)]
    bases = [0, len(per_chunk[0]), len(per_chunk[0])]            # chunk 2 at the base of chunk 1; rightly: + len(per_chunk[1])
    kx, mem = snap["key"]["key_xy"].copy(), snap["key"]["member"].copy()
    for rows, b in zip(per_chunk, bases):
        m = min(len(rows), len(kx) - b)
        kx[b:b + m] = before["key_xy"][rows[:m]]; mem[b:b + m] = before["member"][rows[:m]]
    wrong = dict(snap, key=dict(snap["key"], key_xy=kx, member=mem))
    good = copy.deepcopy(ledger)
    good.step(snap, "the right bases")
    with pytest.raises(C.LedgerError, match="key point changed"):
        ledger.step(wrong, "key-late")


def test_ledger_rejects_a_reused_id_and_a_moved_birth():
    """The ledger's own rules on the table: a used id handed out again, ids that are not consecutive, a birth that changes."""
    rng = np.random.default_rng(24)
    c, ledger = base()
    snap, _ = one_step(c, ledger, 1, status_of("random", rng), rng, 17, S_CPU)
    dropped = next(i for r, i in enumerate(snap["step_ids"]) if not snap["keep"][r])
    ids = snap["ids"].copy(); ids[-1] = dropped
    with pytest.raises(C.LedgerError):
        copy.deepcopy(ledger).step(dict(snap, ids=ids), "reused id")
    ids = snap["ids"].copy(); ids[-1] += 1
    with pytest.raises(C.LedgerError, match="consecutive"):
        copy.deepcopy(ledger).step(dict(snap, ids=ids), "a gap in the ids")
    birth = snap["birth_xy"].copy(); birth[0, 0] += 1
    with pytest.raises(C.LedgerError, match="birth"):
        copy.deepcopy(ledger).step(dict(snap, birth_xy=birth), "moved birth")
    ledger.step(snap, "as it was")


def test_ledger_follows_a_replaced_stream_and_a_held_step():
    """redetect_replace in front of LK: every row starts over with a fresh id, and nothing of the old rows' state may show on them.
    A held step: nothing moves."""
    rng = np.random.default_rng(25)
    c, ledger = base()
    held = c.snapshot(c.padded(c.pos, F, 2), np.zeros((S_CPU, 2), F), np.zeros(S_CPU, np.uint8), c.n, held=True)
    ledger.step(held, "held")
    aged = dict(held, age=held["age"] + 1)
    with pytest.raises(C.LedgerError, match="held"):
        copy.deepcopy(ledger).step(aged, "held, and yet older")
    c.replaced(np.column_stack([rng.uniform(12, WI - 15, 80), rng.uniform(12, HI - 14, 80)]).astype(F))
    snap, info = one_step(c, ledger, 1, np.ones(S_CPU, np.uint8), rng, 0, S_CPU, replaced=True)
    assert info["n_old"] == 80 and c.krec[3] == K.NONE and c.trec[16] == 80 and snap["step_ids"][0] == N
    stale = snap["step_ids"].copy(); stale[0] = 3                # a replaced row that kept an old row's id
    with pytest.raises(C.LedgerError):
        copy.deepcopy(ledger).step(dict(snap, step_ids=stale), "replaced, with a used id")
    old_depth = dict(snap["depth"], nobs=snap["depth"]["nobs"] + 7)     # a replaced row that kept an old row's depth
    with pytest.raises(C.LedgerError, match="observation count"):
        copy.deepcopy(ledger).step(dict(snap, depth=old_depth), "replaced, with an old depth")
    ledger.step(snap, "replaced")
