"""The per-track state with every track setting on, past 512 rows per stream (tests/test_gpu_track_state_counts.py and its CPU
companion tests/test_track_state_cases.py).  Test infrastructure only; the product never imports it.

A stream step queues up to five compactions one behind the other - the keyframe's, the depths', the templates', the table's and the
tracks' own - and each recomputes the same keep prefix in passes of 256 rows.  They agree only if all of them read the status behind
the last of the four drop sources (the gates, the templates, the robust solve, the feasibility keep) and clamp the appended rows by
the same new_counts / max_total.  One row of disagreement moves one feature's state onto the neighbouring track for the rest of the
stream, and every record stays plausible.  Three things here look for that:

Composed    the five numpy restatements (track_table_reference.update, track_depth_reference.step, track_template_reference.
            template_step, keyframe_reference.step / keyframe_rot_reference.step) advanced together for ONE stream from what a step
            hands back.  It knows nothing of a device.
Ledger      a dict per stream keyed by track id, fed with step_ids (the id a row held during the step) and ids (behind it).  It
            restates no kernel: whatever row a surviving id moved to, its track is its next point, its flow next - prev, its age one
            more, its birth unchanged; its template bytes, its key point and its observation count change only in the ways the step's
            own records report.
Follower    Composed and Ledger beside a context's streams: the points in front of the templates come from ofk_lk_pyr_fb on a second
            context, started at track_table_reference.seed_points of the table downloaded before the step; after every call every
            download is compared with the restatements (the comparison helpers and tolerances are the feature tests' own) and fed to
            the ledger.  The largest deviations met are kept in DEV.

Scene: streams 0 and 1 of point_count_cases.stream_frames(), 240 x 320, 8 frames, 600+ corners at quality 0.0005, min_distance 2,
block_size 5.  The context holds S = 704 points per stream: a step that has to land on 600 tracks asks for more corners than that."""
import dataclasses

import numpy as np

import point_count_cases as P
import track_table_reference as TT
import track_depth_reference as TD
import track_template_reference as TP
import keyframe_reference as K
import keyframe_rot_reference as RR
import test_gpu_track_table as GT            # differing / bits, and the comparison helpers of the feature tests below
import test_gpu_track_depth as GD
import test_gpu_track_template as GP
import test_gpu_keyframe as GK
import test_gpu_keyframe_rot as GR
from point_count_cases import bits
from oracle import image_oracle as io

F = np.float32
B, S, NF = 2, 704, P.NF
H, W = P.H, P.W
GAIN = 1.0                                                       # track_table_setting("flow")
TEMPLATE = TP.setting(outside=TP.DROP, anchor_iters=3, ncc_min=0.994, scale_max=1.001)
# Measured on this scene (printed by the GPU tests with -s): the re-anchored windows score 0.998 in the median, 0.996 at the 5 % and 0.992
# - 0.996 at the 1 % quantile, so ncc_min 0.994 fails a few rows of every hundred; the score is a quotient of integer sums, the same bits
# in numpy and on the device, so no decision sits on a rounding.  The scene grows by about 0.1 % per frame: det A is 1.0015 behind a
# track's first scored step and 1.003 behind its second, and scale_max 1.001 (det A <= 1.002) marks it for refresh there.
DEPTH = TD.setting()
KEYFRAME = GK.SET_STREAM
ROTATION = RR.setting(sigma_bias=1e-3)                           # source gyro, no axis held
GATE = dict(fb_thr=0.5, err_max=12.0, **P.VARIANTS["seeded-L0"])    # LK's err is 2.7 in the median and 5 - 10 at the 99 % quantile here: the cap takes a few rows per step
GYRO_ERROR = np.array([1e-3, -5e-4, 8e-4])                       # in the sensors' omega: the rotation has something to refine
ALL_ON = ("template", "depth", "key", "rot")
DEV = dict(depth_rec=0.0, key_rec=0.0, key_R=0.0, rot_rec=0.0, fit=0.0)       # the largest deviations met, in units of their group's scale
TEMPLATE_KEYS = GP.KEYS


def e2_of(cfg=TEMPLATE):
    return (cfg.win + 2) ** 2


# ------------------------------------------------------------------------------------------------ the composed restatement
class Composed:
    """The five restatements of one stream over a stride of S rows.  on: which of "template", "depth", "key", "rot" run beside the
    table.  Every piece starts empty where it is switched on (start / stop), as the device starts it in front of its first step."""

    def __init__(self, S, tracks, template=TEMPLATE, depth=DEPTH, key=KEYFRAME, rot=ROTATION, gain=GAIN, on=ALL_ON):
        self.S, self.cfg, self.ds, self.ks, self.rs, self.gain = S, template, depth, key, rot, gain
        tracks = np.asarray(tracks, F).reshape(-1, 2)
        self.table, self.stats = TT.begin(np.concatenate([tracks, np.zeros((S - len(tracks), 2), F)]), len(tracks), S)
        self.pos = tracks.copy()
        self.tpl = self.depth = self.key = None
        self.trec = self.drec = self.krec = self.rrec = None
        self.rot = False
        for name in on:
            self.start(name)

    @property
    def n(self):
        return self.table["count"]

    def start(self, name):
        if name == "template":
            self.tpl, self.trec = TP.empty_state(self.S, self.cfg.win), None
        elif name == "depth":
            self.depth, self.drec = TD.empty(self.S), None
        elif name == "key":
            self.key, self.krec = RR.empty(self.S), None
        elif name == "rot":
            assert self.key is not None, "the rotation needs the keyframe"
            self.rot, self.rrec = True, None
            self.key["rstate"] = np.zeros(RR.ROT_STATE)

    def stop(self, name):
        if name == "template":
            self.tpl = self.trec = None
        elif name == "depth":
            self.depth = self.drec = None
        elif name == "key":
            self.key = self.krec = self.rrec = None; self.rot = False
        elif name == "rot":
            self.rot, self.rrec = False, None

    def replaced(self, new_pts):
        """redetect_replace in front of LK: fresh rows, every piece's rows empty, the keyframe without members."""
        new_pts = np.asarray(new_pts, F).reshape(-1, 2)
        n = len(new_pts)
        self.table, self.stats = TT.replace(self.table, new_pts, n)
        self.pos = new_pts.copy()
        if self.depth is not None:
            for k in ("rho", "var", "nobs"):
                self.depth[k][:n] = 0
        if self.key is not None:
            self.key["member"][:n] = 0; self.key["key_xy"][:n] = 0; self.key["istate"][1] = 0
            self.key["rstate"] = np.zeros(RR.ROT_STATE)
            self.krec = None                                     # the record is the previous step's: its members_at_key is stale
            if self.rrec is not None:
                self.rrec = np.zeros(RR.ROT_DOUBLES); self.rrec[3] = RR.NONE
        # the templates of rows of age 0 are captured anew whatever their tstate says

    def padded(self, a, dtype, *tail):
        a = np.asarray(a, dtype)
        return np.concatenate([a, np.zeros((self.S - len(a),) + tail, dtype)])

    def templates(self, g0, g1, lk_next, lk_status, L, new_count=None, max_total=None):
        """track_template_reference.template_step on the points behind the gates -> (next [S,2], status [S], state, rec)."""
        n = self.n
        return TP.template_step(g0, g1, self.padded(self.pos, F, 2), lk_next, lk_status, self.table["age"], n, L, self.tpl, self.cfg, new_count, max_total)

    def step(self, lk_next, lk_status, keep, new_pts, max_total, sensors, v, v_uav, solved, g0=None, g1=None, L=None, scored=None,
             depth_keep=None):
        """One step.  lk_next [S,2], lk_status [S]: the points and the status behind the gates, in front of the templates; keep [S]:
        the final keep flags (None: the templates' status - nothing dropped a row behind them); new_pts [m,2]: the appended corners
        (None: no re-detection); sensors [28]; v, v_uav [3], solved: the step record's.  scored: templates() of this step where the
        caller has run it already.  depth_keep: ONLY for the deliberately wrong composition of the CPU tests - the depths compacted
        with another status than everything else.  -> (next [S,2], keep [S]) as every piece read them."""
        n, Sx = self.n, self.S
        prev = self.padded(self.pos, F, 2)
        new_count = None if new_pts is None else len(new_pts)
        nxt, st = np.array(lk_next, F), np.array(lk_status, np.uint8)
        if self.tpl is not None:
            nxt, st, state, self.trec = scored if scored is not None else self.templates(g0, g1, lk_next, lk_status, L, new_count, max_total)
            if keep is not None and np.any((np.asarray(keep)[:n] != 0) != (st[:n] != 0)):
                # the solve dropped rows behind the templates: rule 6 ran on what it left - the same rows scored, fewer kept
                assert not np.any((np.asarray(keep)[:n] != 0) & (st[:n] == 0)), "a row the templates dropped is kept"
                both = ((np.asarray(keep) != 0) & (np.asarray(lk_status) != 0)).astype(np.uint8)
                _, _, state, rec6 = TP.template_step(g0, g1, prev, lk_next, both, self.table["age"], n, L, self.tpl, self.cfg, new_count, max_total)
                self.trec = self.trec.copy(); self.trec[18] = rec6[18]
            self.tpl = state
        keep = st if keep is None else np.asarray(keep, np.uint8)
        kept = int(np.count_nonzero(keep[:n]))
        if self.key is not None:
            if self.rot:
                self.key, self.krec, self.rrec, count, _ = RR.step(self.key, nxt, keep, n, sensors, v_uav, bool(solved), self.table["step"], self.ks,
                                                                   self.rs, new_count=new_count, max_total=max_total)
            else:
                rstate = self.key.get("rstate")
                plain = {k: self.key[k] for k in ("key_xy", "member", "state", "istate")}
                self.key, self.krec, count, _ = K.step(plain, nxt, keep, n, sensors, v_uav, bool(solved), self.table["step"], self.ks,
                                                       new_count=new_count, max_total=max_total)
                if rstate is not None:
                    self.key["rstate"] = rstate
        if self.depth is not None:
            sr = np.asarray(sensors, np.float64)
            x = (nxt.astype(np.float64) - [sr[20], sr[21]]) * sr[19]
            u = (nxt.astype(np.float64) - prev.astype(np.float64)) * sr[19]
            self.depth, self.drec, count, _ = TD.step(self.depth, x, u, keep if depth_keep is None else depth_keep, n, sr[4:7], v, bool(solved),
                                                      self.ds, new_count=new_count, max_total=max_total, scale=sr[19])
        self.table, self.step_ids, self.stats = TT.update(self.table, prev, nxt, keep, new_pts, new_count, max_total, seed=True, gain=self.gain)
        count = self.table["count"]
        self.pos = np.concatenate([nxt[:n][keep[:n] != 0], np.zeros((0, 2), F) if new_pts is None else np.asarray(new_pts, F).reshape(-1, 2)[:count - kept]])
        assert len(self.pos) == count
        return nxt, keep

    def snapshot(self, prev, nxt, keep, n_old, held=False, replaced=False):
        """What the ledger reads, from the restatements' own state (the CPU tests' stand-in for a device's downloads)."""
        c = self.n
        t = self.table
        snap = dict(n_old=n_old, prev=np.asarray(prev, F)[:n_old], next=np.asarray(nxt, F)[:n_old], keep=np.asarray(keep)[:n_old] != 0,
                    step_ids=self.step_ids[:n_old], ids=t["ids"][:c], tracks=self.pos, age=t["age"][:c], birth_xy=t["birth_xy"][:c],
                    birth_step=t["birth_step"][:c], flow_xy=t["flow_xy"][:c], next_id=t["next_id"], step=t["step"], held=held, replaced=replaced)
        if self.tpl is not None:
            snap["template"] = dict(tmpl=self.tpl["tmpl"][:c, :e2_of(self.cfg)], tstate=self.tpl["tstate"][:c], flag=self.tpl["flag"][:c],
                                    refreshed=int(self.trec[18]))
        if self.key is not None:
            snap["key"] = dict(key_xy=self.key["key_xy"][:c], member=self.key["member"][:c], rekey=self.krec[9] != 0, first=self.krec[3] == K.NONE)
        if self.depth is not None:
            snap["depth"] = dict(nobs=self.depth["nobs"][:c], rho=self.depth["rho"][:c], var=self.depth["var"][:c], resets=int(self.drec[20]))
        return snap


# ------------------------------------------------------------------------------------------------ the id ledger
class LedgerError(AssertionError):
    pass


def _need(ok, *what):
    if not ok:
        raise LedgerError(what)


class Ledger:
    """One stream's tracks by id.  begin() with the first table, step() with every later snapshot (Composed.snapshot's keys)."""

    def __init__(self, tag=""):
        self.tag = tag
        self.rows, self.order, self.used, self.next_id = {}, [], set(), 0
        self.moved_down = {256: 0, 512: 0}                       # surviving ids that moved from a row >= the edge to a row below it
        self.straddled = {256: 0, 512: 0}                        # appends with kept < edge < kept + extra

    def begin(self, ids, tracks):
        ids = [int(i) for i in ids]
        _need(len(set(ids)) == len(ids), self.tag, "begin: ids are not unique")
        _need(sorted(ids) == list(range(len(ids))), self.tag, "begin: ids are not 0 .. count - 1")
        self.rows = {i: dict(age=0, birth_xy=np.array(tracks[r], F), birth_step=0, pos=np.array(tracks[r], F)) for r, i in enumerate(ids)}
        self.order, self.used, self.next_id = ids, set(ids), len(ids)

    def _fresh(self, ids, what):
        ids = sorted(int(i) for i in ids)
        _need(ids == list(range(self.next_id, self.next_id + len(ids))), self.tag, what, "fresh ids are not consecutive from next_id", self.next_id, ids[:4])
        _need(not (set(ids) & self.used), self.tag, what, "a used id was handed out again")
        self.used |= set(ids); self.next_id += len(ids)

    def step(self, s, tag=""):
        tag = (self.tag, tag)
        ids = [int(i) for i in s["ids"]]
        at = {i: q for q, i in enumerate(ids)}
        _need(len(at) == len(ids), tag, "ids are not unique")
        pieces = {k: s.get(k) for k in ("template", "key", "depth")}
        if s["held"]:
            return self._held(s, ids, pieces, tag)
        sid = [int(i) for i in s["step_ids"]]
        _need(len(sid) == s["n_old"], tag, "step_ids")
        if s["replaced"]:                                        # every row starts over in front of LK
            _need(len(set(sid)) == len(sid), tag, "replaced: step_ids are not unique")
            self._fresh(sid, "replaced")
            _need(sid == list(range(sid[0], sid[0] + len(sid))) if sid else True, tag, "replaced: step_ids out of row order")
            self.rows = {i: dict(age=0, birth_xy=np.array(s["prev"][r], F), birth_step=int(s["step"]) - 1, pos=np.array(s["prev"][r], F), fresh=True)
                         for r, i in enumerate(sid)}
        else:
            _need(sid == self.order, tag, "step_ids are not the ids the rows held", P.differing(np.array(sid), np.array(self.order))[:4])
        survivors = set()
        with np.errstate(all="ignore"):
            flow = (s["next"] - s["prev"]).astype(F)
        rows = {}
        for r, i in enumerate(sid):
            old = self.rows[i]
            if not s["keep"][r]:
                _need(i not in at, tag, "a dropped id is still in the table", i, r)
                continue
            _need(i in at, tag, "a surviving id is gone", i, r)
            q = at[i]
            survivors.add(i)
            _need(np.array_equal(bits(s["tracks"][q]), bits(s["next"][r])), tag, "a survivor's track is not its next point", i, r, q)
            _need(np.array_equal(bits(s["flow_xy"][q]), bits(flow[r])), tag, "a survivor's flow is not next - prev", i, r, q)
            _need(s["age"][q] == old["age"] + 1, tag, "a survivor's age did not grow by one", i, r, q, s["age"][q], old["age"])
            _need(np.array_equal(bits(s["birth_xy"][q]), bits(old["birth_xy"])) and s["birth_step"][q] == old["birth_step"], tag, "a birth changed", i, r, q)
            for edge in self.moved_down:
                self.moved_down[edge] += int(r >= edge > q)
            rows[i] = dict(age=old["age"] + 1, birth_xy=old["birth_xy"], birth_step=old["birth_step"], pos=np.array(s["tracks"][q], F))
            for name, p in pieces.items():
                if p is not None:
                    getattr(self, "_" + name)(p, q, old, rows[i], i, tag)
        born = [i for i in ids if i not in survivors]
        self._fresh(born, "appended")
        _need(s["next_id"] == self.next_id, tag, "next_id", s["next_id"], self.next_id)
        kept = len(survivors)
        for edge in self.straddled:
            self.straddled[edge] += int(kept < edge < kept + len(born))
        for i in born:
            q = at[i]
            _need(s["age"][q] == 0 and not s["flow_xy"][q].any() and s["birth_step"][q] == s["step"], tag, "an appended row is not new", i, q)
            _need(np.array_equal(bits(s["birth_xy"][q]), bits(s["tracks"][q])), tag, "an appended row was not born where it stands", i, q)
            rows[i] = dict(age=0, birth_xy=np.array(s["tracks"][q], F), birth_step=int(s["step"]), pos=np.array(s["tracks"][q], F))
            p = pieces["template"]
            if p is not None:
                _need(p["tstate"][q] == 0, tag, "an appended row has a template", i, q)
                rows[i]["tstate"], rows[i]["tmpl"] = 0, p["tmpl"][q].copy()
            p = pieces["key"]
            if p is not None:
                _need(p["member"][q] == 0 and not p["key_xy"][q].any(), tag, "an appended row is a member of the keyframe", i, q)
                rows[i]["member"], rows[i]["key_xy"] = 0, p["key_xy"][q].copy()
            p = pieces["depth"]
            if p is not None:
                _need(p["nobs"][q] == 0 and p["rho"][q] == 0 and p["var"][q] == 0, tag, "an appended row has a depth", i, q)
                rows[i]["nobs"] = 0
        # the counts the step's own records report
        p = pieces["template"]
        if p is not None:
            lost = sum(1 for i in survivors if rows[i]["tstate"] == 0 and (self.rows[i].get("tstate", 0) != 0 or rows[i]["captured"]))
            _need(lost == p["refreshed"], tag, "templates went from 1 to 0 where the refresh count does not say so", lost, p["refreshed"])
        p = pieces["depth"]
        if p is not None:
            fell = sum(1 for i in survivors if rows[i]["nobs"] < self.rows[i].get("nobs", 0))
            _need(fell <= p["resets"], tag, "more observation counts fell than the record's resets", fell, p["resets"])
        self.rows, self.order = rows, ids

    # the pieces of a survivor: p the piece's snapshot, q its row now, old / new the id's entries before and behind the step
    def _template(self, p, q, old, new, i, tag):
        ts, flag = int(p["tstate"][q]), int(p["flag"][q])
        captured = bool(flag & TP.CAPTURED)
        had = "tstate" in old and old["tstate"] != 0 and not old.get("fresh")
        if "tstate" not in old or old.get("fresh"):              # the piece's (or the row's) first step: whatever it holds was captured now
            _need(ts == 0 or captured, tag, "a template that no step captured", i, q)
        elif not captured:
            _need(had or ts == 0, tag, "a template appeared without a capture", i, q)
            _need(not had or np.array_equal(p["tmpl"][q], old["tmpl"]), tag, "template bytes changed in a step that did not capture them", i, q)
        new["tstate"], new["tmpl"], new["captured"] = ts, p["tmpl"][q].copy(), captured

    def _key(self, p, q, old, new, i, tag):
        if "key_xy" not in old or old.get("fresh"):
            _need(p["rekey"] and p["first"], tag, "a keyframe state without a first keying", i, q)
        if p["rekey"]:
            _need(p["member"][q] == 1 and np.array_equal(bits(p["key_xy"][q]), bits(new["pos"])), tag, "a re-key did not take the survivor's point", i, q)
        else:
            _need(np.array_equal(bits(p["key_xy"][q]), bits(old["key_xy"])) and p["member"][q] == old["member"], tag,
                  "a key point changed in a step that reports no re-key", i, q)
        new["key_xy"], new["member"] = p["key_xy"][q].copy(), int(p["member"][q])

    def _depth(self, p, q, old, new, i, tag):
        was = 0 if old.get("fresh") else old.get("nobs", 0)
        now = int(p["nobs"][q])
        _need(now - was in (0, 1) or now == 0, tag, "an observation count moved by something else than 0, +1 or a reset", i, q, was, now)
        new["nobs"] = now

    def _held(self, s, ids, pieces, tag):
        """A held step changes no id's state but for the templates it captured for rows that had none."""
        _need(not s["replaced"], tag, "held: a replace in front of a held step is not followed here")
        _need(ids == self.order and s["next_id"] == self.next_id, tag, "held: the ids moved")
        for q, i in enumerate(ids):
            old = self.rows[i]
            _need(s["age"][q] == old["age"] and np.array_equal(bits(s["tracks"][q]), bits(old["pos"])), tag, "held: a track moved or aged", i, q)
            _need(np.array_equal(bits(s["birth_xy"][q]), bits(old["birth_xy"])) and s["birth_step"][q] == old["birth_step"], tag, "held: a birth changed", i, q)
            p = pieces["template"]
            if p is not None and "tstate" in old:
                if old["tstate"] != 0:
                    _need(p["tstate"][q] == old["tstate"] and np.array_equal(p["tmpl"][q], old["tmpl"]), tag, "held: a template changed", i, q)
                else:
                    old["tstate"], old["tmpl"] = int(p["tstate"][q]), p["tmpl"][q].copy()
            p = pieces["key"]
            if p is not None and "key_xy" in old:
                _need(np.array_equal(bits(p["key_xy"][q]), bits(old["key_xy"])) and p["member"][q] == old["member"], tag, "held: a key point changed", i, q)
            p = pieces["depth"]
            if p is not None and "nobs" in old:
                _need(p["nobs"][q] == old["nobs"], tag, "held: an observation count changed", i, q)


# ------------------------------------------------------------------------------------------------ beside a device
OBJECT = dict(size=(48, 64), at=(60, 210), step=(2, -3))          # rows, columns; per frame


def frames_and_sensors(blank=False, nb=B, moving=False):
    """The first nb streams of point_count_cases.stream_frames and their sensor rows.  moving: a textured rectangle moves over every
    stream's ground by OBJECT["step"] per frame (robust_reference.scene's object, as point_count_cases.pair_scenes pastes it).  On
    the rigid scene alone the forward-backward gate and the templates leave the robust solve no row of weight 0 to drop (measured: 0 in
    14 stream steps); the tracks on the object pass the gates and the templates and are the solve's to drop."""
    frames, info = P.stream_frames(blank)
    frames = frames[:nb]
    if moving:
        frames = frames.copy()
        (oh, ow), (r, c), (dr, dc) = OBJECT["size"], OBJECT["at"], OBJECT["step"]
        for b in range(nb):
            tex = P.synth().render_pair(oh + 40, ow + 40, 140 + b, margin=96)["prev"][20:20 + oh, 20:20 + ow]
            for t in range(frames.shape[1]):
                frames[b, t, r + dr * t:r + dr * t + oh, c + dc * t:c + dc * t + ow] = tex
    sensors = P.sensor_rows(info, nb)
    sensors[:, 4:7] += GYRO_ERROR
    return frames, sensors


def device_settings(ofk):
    return dict(table=ofk.track_table_setting("flow", GAIN), depth=ofk.track_depth_setting(), template=GP.device_setting(ofk, TEMPLATE),
                key=GK.device_setting(ofk, KEYFRAME), rot=GR.device_rot(ofk, ROTATION),
                gate=ofk.track_gate_setting(fb=GATE["fb"], fb_thr=GATE["fb_thr"], fb_level=GATE["fb_level"], err_max=GATE["err_max"]))


def switch(ctx, ofk, name, on):
    s = device_settings(ofk)
    {"depth": ctx.set_track_depth, "template": ctx.set_track_template, "key": ctx.set_keyframe, "rot": ctx.set_keyframe_rotation}[name](s[name] if on else None)


def open_context(ofk, nb, cfg, on=ALL_ON, robust=False, zones=False, fused=False):
    ctx = ofk.Context(0, W, H, nb, S, cfg.max_level)
    s = device_settings(ofk)
    if robust:
        ctx.set_robust(cfg.robust_setting())
    if zones:
        ctx.set_zones(ofk.zones_setting("hull"))
    if fused:
        ctx.imu_reset(nb)
    ctx.set_track_gate(s["gate"])
    ctx.set_track_table(s["table"])
    for name in on:
        switch(ctx, ofk, name, True)
    return ctx


def downloads(ctx, nb, on):
    """Every per-track download of a context, for the bit comparison of two runs."""
    out = dict(table=ctx.track_table_download(nb, S))
    out["last"] = dict(zip(("next", "keep"), ctx.stream_last_points(S)))
    if "depth" in on:
        out["depth"] = ctx.track_depth_download(nb, S)
    if "template" in on:
        out["template"] = ctx.track_template_download(nb, S)
    if "key" in on:
        out["key"] = ctx.keyframe_download(nb, S)
    if "rot" in on:
        out["rot"] = dict(rec=ctx.keyframe_rotation_download(nb))
    return out


class Follower:
    """Composed and Ledger per stream beside the streams of `ctx`; `stage` is a second context for ofk_lk_pyr_fb and the step map."""

    def __init__(self, ofk, ctx, stage, cfg, sensors, tracks, counts, on=ALL_ON, fused=False, solve_drops=False):
        """fused: the calls are ofk_stream_step_fused's.  solve_drops: the solve may drop rows behind the templates (the robust drop);
        without it the final keep flags are asserted to be the status behind the gates and the templates, row for row."""
        self.ofk, self.ctx, self.stage, self.cfg, self.sensors, self.fused, self.solve_drops = ofk, ctx, stage, cfg, sensors, fused, solve_drops
        self.nb = len(counts)
        self.on = set(on)
        self.c = [Composed(S, tracks[b, :counts[b]], on=on) for b in range(self.nb)]
        self.ledger = [Ledger(("stream", b)) for b in range(self.nb)]
        d = ctx.track_table_download(self.nb, S)
        for b in range(self.nb):
            self.compare_table(d, b, "begin")
            self.ledger[b].begin(d["ids"][b, :counts[b]], tracks[b, :counts[b]])
        self.gate = device_settings(ofk)["gate"]
        self.seen = dict(n_old=[], refused=0, template_drops=0, refreshed=0, solve_drops=0, rekeys_later=0, map_solves=0, held=0, replaced=0,
                         zero_rows=0, captured=0, resets=0)

    def start(self, name):
        self.on.add(name)
        for c in self.c:
            c.start(name)

    def stop(self, name):
        self.on.discard(name)
        for c in self.c:
            c.stop(name)

    # ---- in front of a step
    def look(self, next_bgr, replace=None):
        """The points behind the gates and in front of the templates, as the step about to run will see them: ofk_lk_pyr_fb on the
        second context from the resident previous frame and the new frame's gray, started at the table's seeds.  replace: (min_features,
        max_corners) of a redetect_replace step - the streams with few tracks start over with the corners of the previous frame."""
        nb, cfg = self.nb, self.cfg
        g0 = np.stack([self.ctx.resident_pyramid(0, b, H, W, 0)[0] for b in range(nb)])
        g1 = self.stage.gray_bgr8(next_bgr)
        self.was_replaced = [False] * nb
        if replace is not None:
            mf, mc = replace
            for b, c in enumerate(self.c):                       # k_redetect_limits' rule, the detection of the reference loop
                if c.n <= mf and mc - c.n > 0:
                    c.replaced(io.good_features(g0[b], mc - c.n, cfg.quality, cfg.min_distance, cfg.block_size).reshape(-1, 2))
                    self.was_replaced[b] = True
        n_old = [c.n for c in self.c]
        prev = np.stack([c.padded(c.pos, F, 2) for c in self.c])
        init = np.stack([TT.seed_points(prev[b], n_old[b], c.table["age"], c.table["flow_xy"], GAIN) for b, c in enumerate(self.c)])
        lk = self.stage.lk_pyr_fb(g0, g1, prev, n_old, self.gate, cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr, next_pts=init,
                                  flags=self.ofk.LK_USE_INITIAL_FLOW)
        fit = L = None
        if "template" in self.on:
            fit, L = self.stage.track_affine_fit(prev, lk["next_pts"], lk["status"], n_old, H, W, GP.device_setting(self.ofk, TEMPLATE))
        self.ahead = dict(g0=g0, g1=g1, prev=prev, n_old=n_old, lk=lk, fit=fit, L=L)
        return self.ahead

    def will_keep(self, b):
        """How many rows of stream b the gates and the templates will keep (on a plain step: the final keep)."""
        a = self.ahead
        if "template" not in self.on:
            return int(np.count_nonzero(a["lk"]["status"][b, :a["n_old"][b]]))
        st = self.c[b].templates(a["g0"][b], a["g1"][b], a["lk"]["next_pts"][b], a["lk"]["status"][b], a["L"][b])[1]
        return int(np.count_nonzero(st[:a["n_old"][b]]))

    # ---- behind a step
    def compare_table(self, d, b, tag, step_ids=True):
        c = self.c[b]
        n = c.n
        assert np.array_equal(d["stats"][b], c.stats), (tag, b, "table stats", d["stats"][b], c.stats)
        for k in GT.KEYS:
            assert np.array_equal(bits(d[k][b, :n]), bits(c.table[k][:n])), (tag, b, k, P.differing(d[k][b, :n], c.table[k][:n])[:4])
        if step_ids and hasattr(c, "step_ids"):
            assert np.array_equal(d["step_ids"][b, :len(c.step_ids)], c.step_ids), (tag, b, "step_ids")

    def step(self, rec, tracks, counts, max_total, tag, held=False):
        """Behind the device's call: advance the restatements with what it handed back, compare every download, feed the ledgers."""
        ctx, nb, a = self.ctx, self.nb, self.ahead
        nxt_dev, keep_dev = ctx.stream_last_points(S)
        d = downloads(ctx, nb, self.on)
        slot = (0, 1) if held else (1, 0)                        # a step that is not held swaps the frames behind it
        for b in range(nb):
            assert np.array_equal(ctx.resident_pyramid(slot[0], b, H, W, 0)[0], a["g0"][b]), (tag, b, "the previous frame")
            assert np.array_equal(ctx.resident_pyramid(slot[1], b, H, W, 0)[0], a["g1"][b]), (tag, b, "the new frame's gray")
        gstats = ctx.track_gate_stats(nb)
        for b, c in enumerate(self.c):
            n_old = a["n_old"][b]
            lk_next, lk_status = a["lk"]["next_pts"][b], a["lk"]["status"][b]
            keep = keep_dev[b]
            kept = int(np.count_nonzero(keep[:n_old]))
            sr = self.sensors[b]
            solved = rec[b, 15] != 0 if self.fused else rec[b, 4] >= 3
            assert rec[b, 12] == n_old, (tag, b, "the rows the step tracked", rec[b, 12], n_old)
            self.seen["n_old"].append(n_old)
            self.seen["zero_rows"] += int(n_old == 0)
            self.seen["refused"] += int(np.sum(gstats[b][1:4]))          # lost in the backward pass, far, capped
            if "template" in self.on:                            # the device's own step map is the second context's, and the restatement's to rounding
                want, _ = TP.affine_fit(a["prev"][b], lk_next, lk_status, n_old, H, W, TEMPLATE)
                got = d["template"]["rec"][b]
                err = float((np.abs(got[:10] - want[:10]) / np.maximum(1.0, np.abs(want[:10]))).max())
                DEV["fit"] = max(DEV["fit"], err)
                assert np.array_equal(got[[6, 7]], want[[6, 7]]) and err <= 1e-10, (tag, b, "step map", got[:10], want[:10])
                assert np.array_equal(bits(got[:10]), bits(a["fit"][b, :10])) and np.array_equal(bits(got[0:4].astype(F)), bits(a["L"][b])), (tag, b, "step map")
            if held:
                self.held(d, b, nxt_dev[b], tag)
                continue
            new_pts = tracks[b, kept:counts[b]]
            grays = dict(g0=a["g0"][b], g1=a["g1"][b], L=None if a["L"] is None else a["L"][b])
            scored = None
            if "template" in self.on:                            # with the step's own new_count, whatever will_keep scored in front of it
                scored = c.templates(grays["g0"], grays["g1"], lk_next, lk_status, grays["L"], len(new_pts), max_total)
            nxt, _ = c.step(lk_next, lk_status, keep, new_pts, max_total, sr, rec[b, 0:3], rec[b, 8:11], solved, scored=scored, **grays)
            assert c.n == counts[b], (tag, b, "count", c.n, counts[b])
            assert np.array_equal(bits(nxt_dev[b, :n_old]), bits(nxt[:n_old])), (tag, b, "next", P.differing(nxt_dev[b, :n_old], nxt[:n_old])[:4])
            assert np.array_equal(bits(tracks[b, :kept]), bits(nxt[:n_old][keep[:n_old] != 0])), (tag, b, "the kept tracks are the next points")
            st = scored[1] if "template" in self.on else lk_status  # the status in front of the solve
            assert not np.any((keep[:n_old] != 0) & (st[:n_old] == 0)), (tag, b, "a row the gates or the templates dropped is kept")
            dropped = np.flatnonzero((keep[:n_old] == 0) & (st[:n_old] != 0))
            assert self.solve_drops or not len(dropped), (tag, b, "rows dropped behind the templates where nothing drops any", dropped[:6])
            self.seen["solve_drops"] += len(dropped)
            self.compare(d, b, tag)
            self.ledger[b].step(self.snapshot(d, b, a["prev"][b], nxt_dev[b], keep, n_old, tracks[b, :counts[b]], replaced=self.was_replaced[b]), tag)
            self.seen["replaced"] += int(self.was_replaced[b])
        self.seen["held"] += int(held)
        self.last = d
        return d

    def compare(self, d, b, tag):
        c, n = self.c[b], self.c[b].n
        self.compare_table(d["table"], b, tag)
        if "depth" in self.on:
            for k in GD.KEYS:
                assert np.array_equal(GD.bits(d["depth"][k][b, :n]), GD.bits(c.depth[k][:n])), (tag, b, "depth", k, P.differing(d["depth"][k][b, :n], c.depth[k][:n])[:4])
            theirs = list(GD.DEV); GD.DEV[0] = 0.0
            GD.same_record(d["depth"]["rec"][b], c.drec, (tag, b, "depth"))
            DEV["depth_rec"] = max(DEV["depth_rec"], GD.DEV[0]); GD.DEV[:] = theirs
            self.seen["map_solves"] += int(d["depth"]["rec"][b, 3] == 0)
            self.seen["resets"] += int(d["depth"]["rec"][b, 20])
        if "template" in self.on:
            GP.same_state({k: d["template"][k][b] for k in TEMPLATE_KEYS}, c.tpl, n, TEMPLATE.win, (tag, b))
            assert np.array_equal(d["template"]["rec"][b, 10:], c.trec[10:]), (tag, b, "template record", d["template"]["rec"][b, 10:20], c.trec[10:20])
            r = d["template"]["rec"][b]
            self.seen["template_drops"] += int(r[11]); self.seen["refreshed"] += int(r[18]); self.seen["captured"] += int(r[16])
        if "key" in self.on:
            k = d["key"]
            assert np.array_equal(bits(k["key_xy"][b, :n]), bits(c.key["key_xy"][:n])), (tag, b, "key_xy", P.differing(k["key_xy"][b, :n], c.key["key_xy"][:n])[:4])
            assert np.array_equal(k["member"][b, :n], c.key["member"][:n]), (tag, b, "member")
            theirs = dict(GK.DEV); GK.DEV.update(rec=0.0, R=0.0)
            err = float(np.abs(k["R_acc"][b].ravel() - c.key["state"][:9]).max())
            assert err <= GK.R_TOL, (tag, b, "R_acc", k["R_acc"][b], c.key["state"][:9])
            DEV["key_R"] = max(DEV["key_R"], err)
            if c.krec is not None:
                GK.same_record(k["rec"][b], c.krec, (tag, b, "keyframe"))
                self.seen["rekeys_later"] += int(k["rec"][b, 9] != 0 and k["rec"][b, 3] != K.NONE)
            DEV["key_rec"] = max(DEV["key_rec"], GK.DEV["rec"]); GK.DEV.update(theirs)
            c.key["state"][:9] = k["R_acc"][b].ravel()           # R_acc is compared step by step: the next step starts from the device's
            if "rot" in self.on and c.rrec is not None:
                theirs = dict(GR.DEV); GR.DEV.update(rrec=0.0)
                GR.same_rrec(d["rot"]["rec"][b], c.rrec, (tag, b, "rotation"))
                DEV["rot_rec"] = max(DEV["rot_rec"], GR.DEV["rrec"]); GR.DEV.update(theirs)

    def held(self, d, b, nxt_dev, tag):
        """A held step launches no update: every download stays, but for the templates the step captured for rows that had none."""
        c, a = self.c[b], self.ahead
        n = c.n
        self.compare_table(d["table"], b, (tag, "held"), step_ids=False)
        for name in ("depth", "key", "rot"):                     # the records of the last step that was not held stay
            if name in self.on and name in getattr(self, "last", {}):
                assert np.array_equal(bits(d[name]["rec"][b]), bits(self.last[name]["rec"][b])), (tag, b, "held", name, "record")
        if "depth" in self.on:
            for k in GD.KEYS:
                assert np.array_equal(GD.bits(d["depth"][k][b, :n]), GD.bits(c.depth[k][:n])), (tag, b, "held", k)
        if "key" in self.on:
            assert np.array_equal(bits(d["key"]["key_xy"][b, :n]), bits(c.key["key_xy"][:n])) and np.array_equal(d["key"]["member"][b, :n], c.key["member"][:n]), (tag, b, "held")
        if "template" in self.on:
            t = d["template"]
            scored = c.templates(a["g0"][b], a["g1"][b], a["lk"]["next_pts"][b], a["lk"]["status"][b], a["L"][b])
            assert np.array_equal(bits(nxt_dev[:n]), bits(scored[0][:n])), (tag, b, "held: next")
            had = np.flatnonzero(c.tpl["tstate"][:n] != 0)
            for k in TEMPLATE_KEYS:
                assert np.array_equal(t[k][b][had], c.tpl[k][had]), (tag, b, k, "held")
            for r in np.flatnonzero((c.tpl["tstate"][:n] == 0) & (t["tstate"][b, :n] != 0)):
                # a row without a template that the held step captured: the bits the next step would have captured
                assert np.array_equal(t["tmpl"][b, r, :e2_of()], TP.capture(a["g0"][b], a["prev"][b, r, 0], a["prev"][b, r, 1], TEMPLATE.win)), (tag, b, r, "held capture")
                assert np.array_equal(t["A"][b, r], np.array([1, 0, 0, 1], F)), (tag, b, r)
                for k in ("tmpl", "A", "tstate"):
                    c.tpl[k][r] = t[k][b, r]
        self.ledger[b].step(self.snapshot(d, b, a["prev"][b], nxt_dev, np.zeros(S, np.uint8), n, c.pos, held=True, replaced=self.was_replaced[b]), (tag, "held"))

    def snapshot(self, d, b, prev, nxt, keep, n_old, tracks, held=False, replaced=False):
        """The ledger's view of the DEVICE's downloads (Composed.snapshot's keys)."""
        t = d["table"]
        c = int(t["stats"][b, 0])
        snap = dict(n_old=n_old, prev=prev[:n_old], next=nxt[:n_old], keep=keep[:n_old] != 0, step_ids=t["step_ids"][b, :n_old], ids=t["ids"][b, :c],
                    tracks=np.asarray(tracks, F)[:c], age=t["age"][b, :c], birth_xy=t["birth_xy"][b, :c], birth_step=t["birth_step"][b, :c],
                    flow_xy=t["flow_xy"][b, :c], next_id=int(np.uint32(t["stats"][b, 6])), step=int(t["stats"][b, 5]), held=held, replaced=replaced)
        if "template" in self.on:
            p = d["template"]
            snap["template"] = dict(tmpl=p["tmpl"][b, :c, :e2_of()], tstate=p["tstate"][b, :c], flag=p["flag"][b, :c], refreshed=int(p["rec"][b, 18]))
        if "key" in self.on:
            p = d["key"]
            snap["key"] = dict(key_xy=p["key_xy"][b, :c], member=p["member"][b, :c], rekey=p["rec"][b, 9] != 0, first=p["rec"][b, 3] == K.NONE)
        if "depth" in self.on:
            p = d["depth"]
            snap["depth"] = dict(nobs=p["nobs"][b, :c], rho=p["rho"][b, :c], var=p["var"][b, :c], resets=int(p["rec"][b, 20]))
        return snap


def landing(land, n_old, kept):
    """point_count_cases.stream_run's rule: the budget that makes stream 0 end on `land` tracks when its detector fills it."""
    mc = land + n_old - kept
    return mc, mc


def step_cfg(cfg, mc):
    return dataclasses.replace(cfg, max_corners=mc)
