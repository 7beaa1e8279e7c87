"""The stream and pair runs with several settings switched on at once: the cases, their reference loops (stream_oracle.NodeLoop /
oracle_of_module with the plugs composed, batch_oracle.combined_chain) and the counters that show a run active in every setting it
switches on.  tests/test_combined_reference.py runs the references alone and pins the counters; tests/test_gpu_settings_combined.py
compares the device with them step by step.  Test infrastructure only.

The operating point is that of tests/test_gpu_zones.py: robust_stream_oracle.sequence at 480 x 640, seeds 900 and 901, 200 corners,
min_features 199 (every step re-detects), mask radius 15."""
import numpy as np

import corner_grid_reference as cg
import cov_reference as cr
import lk_seed_reference as ls
import robust_stream_oracle as rso
import track_gate_reference as tg
from stream_oracle import NodeLoop, feasibility_solve, imu_messages, oracle_of_module

H, W, NB, NF = 480, 640, 2, 8
SEEDS = (900, 901)
MIN_FEAT, RADIUS = 199, 15
BASE = dict(max_corners=200, quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)
ROBUST = dict(robust="tukey", robust_c=rso.SETTING["c"], robust_iters=rso.SETTING["iters"], robust_hypotheses=rso.SETTING["hypotheses"],
              robust_seed=rso.SETTING["seed"], robust_drop=True)
SEED = dict(lk_seed="model", seed_gain=1.0)
# the backward pass on level 0 alone from the original point, and a cap on LK's err (the mean absolute window difference, gray levels)
GATE = dict(fb_check="seeded", fb_thr=0.05, fb_level=0, err_max=6.0)
# 16 x 12 cells of 40 pixels with one corner each: fewer cells than corners asked for, so the cap decides every selection
GRID = dict(grid_cell=40, grid_cap=1, grid_max_rank=0)
COV = dict(cov="propagate", sigma_flow_px=0.3, sigma_pos_px=0.5, sigma_d=0.04, sigma_omega=(0.01, 0.02, 0.015), sigma_normal=0.004, sigma_offset=0.006)
# the filter's correct takes R_eff = C_uav + r_floor I; NIS_MAX lies between the steps' NIS values (test_combined_reference.py pins them)
NIS_MAX = 3.0
COV_FILTER = dict(COV, cov_filter=True, r_floor=1e-8, nis_max=NIS_MAX)
ZONES = dict(zones="hull")
FEAS_T = 0.04                                                    # r_tilde <= FEAS_T: most of the object's points and few others fail it
OFFSET = (0.02, -0.01, 0.2)
EKF = dict(dt=0.1, r=1e-4, p0=1e-4)

# kind: "step" = FlowStream.step, "fused" = step_fused on the sensors, "ekf6" = step_fused on the resident IMU state with the filter
CASES = {
    "all-fused": dict(kind="ekf6", cfg=dict(BASE, **SEED, **GATE, **GRID, **ROBUST, **COV_FILTER, **ZONES)),
    "all-step": dict(kind="step", cfg=dict(BASE, **SEED, **GATE, **GRID, **ROBUST, **COV, **ZONES)),
    "grid-zones": dict(kind="step", cfg=dict(BASE, **GRID, **ROBUST, **ZONES)),
    "gate-zones": dict(kind="step", cfg=dict(BASE, **GATE, **ROBUST, **ZONES)),
    "seed-gate-robust": dict(kind="step", cfg=dict(BASE, **SEED, **GATE, **ROBUST)),
    "feasibility": dict(kind="fused", cfg=dict(BASE, use_feasibility=True, feas_T=FEAS_T, **ZONES)),
}
_seq = {}


def sequences(synth, nf=NF):
    """The two streams' frames [NB, nf, H, W, 3] and the scene's info, rendered once per process."""
    if nf not in _seq:
        seqs = [rso.sequence(synth, H, W, s, nf) for s in SEEDS]
        _seq[nf] = (np.stack([s[0] for s in seqs]), seqs[0][1])
    return _seq[nf]


def sensor_rows(ofk, info, nb=NB):
    return ofk.make_sensors(nb, d=info["d"], normal=info["n"], omega=info["omega"], offset=OFFSET, scaling=info["scaling"], cx=info["cx"],
                            cy=info["cy"], v_prior=info["v"])


def imu_state0(info):
    """The resident IMU state the ekf6 case starts from: the node's initial values with the true velocity in the place of 0.1."""
    st = np.array([0.1, 0.1, 0.1, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0], np.float64)
    st[0:3] = info["v"]
    return st


def imu_batch(t, nb=NB):
    """The messages [nb, 3, 15] the streams receive before frame t."""
    return np.stack([imu_messages(np.random.default_rng(7000 + 10 * t + b), 50.0 + 0.1 * t + 3 * b, 3, rate=rso.MOTION["omega"], rate_sigma=0.0005)
                     for b in range(nb)])


def gate_of(cfg):
    return tg.setting(fb=cfg.fb_check, fb_thr=cfg.fb_thr, fb_level=cfg.fb_level, err_max=cfg.err_max)


def grid_of(cfg):
    return (cfg.grid_cell, cfg.grid_cap, cfg.grid_max_rank)


def cov_dict(cfg):
    """cov_reference's cfg of a PipelineConfig (mode as cov_reference's integer)."""
    return dict(mode=dict(off=cr.OFF, propagate=cr.PROPAGATE, residual=cr.RESIDUAL)[cfg.cov], sigma_flow=cfg.sigma_flow_px, sigma_pos=cfg.sigma_pos_px,
                sigma_d=cfg.sigma_d, sigma_omega=cfg.sigma_omega, sigma_normal=cfg.sigma_normal, sigma_offset=cfg.sigma_offset,
                filter_r=cfg.cov_filter, r_floor=cfg.r_floor, nis_max=cfg.nis_max, omega_from_imu=cfg.omega_from_imu)


class Reference:
    """The composed reference loops of one case, one per stream, with the logs the comparison and the activity counters need.
    predict: the seed predictor (None: lk_seed_reference.predict).  reject_status: "gated" (ofk.h) or, the deliberately wrong
    reference of the tests' self-check, "forward" = the zone update sees the status ahead of the gates."""

    def __init__(self, name, make_cfg, frames, info, sr, predict=None, reject_status="gated"):
        case = CASES[name]
        self.name, self.kind, self.frames, self.info, self.sr = name, case["kind"], frames, info, sr
        self.cfg = cfg = make_cfg(**case["cfg"])
        nb = len(frames)
        self.gate_log = [[] for _ in range(nb)]; self.grid_log = [[] for _ in range(nb)]
        self.seeded, self.gated, self.grid_on = cfg.lk_seed != "off", cfg.track_gate_setting() is not None, cfg.grid_cell > 0
        self.robust_on, self.cov_on, self.zones_on = cfg.robust != "off", cfg.cov != "off", cfg.zones == "hull"
        self.counters = dict(inserted=0, refreshed=0, masked=0, refused=0, refused_with_rejects=0, dropped=0, examined=0, accepted=0,
                             grid_bound=0, seeded=0, nis_gated=0, nis_steps=0, cov_records=0, solved=0, rejects=0)
        self.loops = []
        for b in range(nb):
            kw = {}
            if self.seeded or self.gated:
                mode = ls.SEED_MODEL if cfg.lk_seed == "model" else ls.SEED_ROTATION if cfg.lk_seed == "rotation" else 0
                kw["lk_src"] = tg.seeded_gated_lk(cfg, gate_of(cfg), mode, cfg.seed_gain, self.gate_log[b], predict)
            if self.grid_on:
                kw["detect"] = cg.grid_detect(cfg, grid_of(cfg), self.grid_log[b])
            if self.robust_on:
                kw["solve"] = rso.robust_solver(b, cfg.robust_drop, self.kind != "step")
            elif cfg.use_feasibility:
                kw["solve"] = feasibility_solve(sr[b, 22:25], cfg.feas_T, 2 if self.kind != "step" else 0)
            if self.zones_on:
                kw["zones"] = {}
            if self.kind == "ekf6":
                kw["imu_offset"] = OFFSET
            loop = NodeLoop(frames[b, 0], cfg, MIN_FEAT, RADIUS, **kw)
            if self.kind == "ekf6":
                loop.imu["vel"] = np.array(info["v"], np.float64)
            if reject_status == "forward":
                loop.zr = _ForwardStatus(loop.zr, self.gate_log[b])
            self.loops.append(loop)
        self.first_grid = [list(lg) for lg in self.grid_log]
        self.filters = None
        if self.kind == "ekf6" and self.cov_on:
            from of_amd.pipeline import FusionConfig
            self.fusion = FusionConfig.ekf6(**EKF)
            self.filters = [cr.CovStreamLoop(self.fusion.model, cov_dict(cfg), self.fusion.z_sign, self.fusion.z_source) for _ in range(nb)]

    def step(self, t, b, msgs=(), src=None):
        """Stream b's step onto frame t -> NodeLoop's dict plus gate (the tracker's full result), grid (accepted, examined) of the
        re-detection, refused (forward status 1, gated status 0), dropped (tracked, not kept)."""
        loop, c = self.loops[b], self.counters
        n_gate, n_grid = len(self.gate_log[b]), len(self.grid_log[b])
        o = loop.step(self.frames[b, t], self.sr[b], msgs, src=src)
        o["gate"] = self.gate_log[b][-1] if len(self.gate_log[b]) > n_gate else None
        o["grid"] = self.grid_log[b][-1] if len(self.grid_log[b]) > n_grid else None
        o["refused"] = 0 if o["gate"] is None else int(np.count_nonzero((o["gate"]["st_f"] == 1) & (o["gate"]["status"] == 0)))
        o["dropped"] = o["n_tracked"] - int(np.count_nonzero(o["keep"]))
        if self.robust_on:
            assert o["gap"] >= 1e-6 and o["near"] == 0, (self.name, t, b, o["gap"], o["near"])      # no near-tie anywhere: no allowance needed
        c["refused"] += o["refused"]; c["dropped"] += o["dropped"]; c["solved"] += int(o["solved"])
        if o["gate"] is not None and self.seeded:
            c["seeded"] += 1
        if o["grid"] is not None:
            c["accepted"] += o["grid"][0]; c["examined"] += o["grid"][1]; c["grid_bound"] += int(o["grid"][1] > o["grid"][0])
        if self.zones_on:
            z = o["zones"]
            c["inserted"] += int(z.stats[1]); c["refreshed"] += int(z.stats[2]); c["rejects"] += int(z.stats[4])
            c["masked"] += int(o["redetected"] and o["zones_masked"] > 0)
            c["refused_with_rejects"] += int(o["refused"] > 0 and z.stats[4] > 0)
        return o

    def cov_record(self, b, o, rec=None, weights=None, imu=None, control=None):
        """The step's cov record (and, with the filter, its x, P, fused) from the reference's points.  rec: the result record that
        supplies v, RSS, rank, v_uav and the solved flag (None: the reference's own); weights likewise; imu: the IMU state row
        (None: built from the loop's own motion source); control: the filter's input (None: the loop's own velocity increments)."""
        R, nrm, om, offset = o["motion"]
        if rec is None:
            rec = np.zeros(16)
            if o["v"] is not None:
                rec[0:3], rec[3], rec[4], rec[8:11], rec[15] = o["v"], o.get("rss", 0.0), o.get("rank", 3), o["v_uav"], 1.0 if o["solved"] else 0.0
        w = o.get("weights") if weights is None else weights
        if self.filters is not None:
            if imu is None:
                imu = np.zeros(24); imu[6:15] = R.ravel(); imu[15:18] = nrm; imu[18:21] = om
            cv, x, P, fused = self.filters[b].step(o["old"], o["new"], o["keep"], self.sr[b], rec, o["dv"] if control is None else control, imu=imu, w=w)
            self.counters["nis_steps"] += int(rec[15] != 0); self.counters["nis_gated"] += int(cv[15])
        else:
            cv, x, P, fused = cr.pair_record(cr.NODE, o["old"], o["new"], None, self.sr[b], cov_dict(self.cfg), rec, w=w, keep=np.asarray(o["keep"], bool)), None, None, None
        self.counters["cov_records"] += int(cv[13] == 0)
        return cv, x, P, fused


class _ForwardStatus:
    """zones_reference with the update fed the status AHEAD of the gates: the wrong reading of rule 1 (a gate-refused point counted
    as a reject) that the gate + zones comparison must tell from the right one."""

    def __init__(self, zr, log):
        self._zr, self._log = zr, log

    def __getattr__(self, k):
        return getattr(self._zr, k)

    def update(self, table, s, old, new, status, keep):
        return self._zr.update(table, s, old, new, self._log[-1]["st_f"] if len(old) else status, keep)


# ---------------------------------------------------------------------------------------- the of_module loop (legacy keep, held step)
OFM = dict(max_corners=60, quality=0.02, block_size=7, min_distance=12, feas_T=-0.5)    # enough corners on the synthetic texture; T keeps most
OFM_MIN_FEAT = 55                                                # the replacing re-detection fires on most steps
OFM_ZONES = dict(link=64, min_members=2)                         # the legacy keep refuses few points per step: pairs of them make a zone
OFM_GRID = (80, 2, 0)
HELD_STEP = 4                                                    # the control of this step throws the predicted velocity far off: nothing is feasible
HELD_CONTROL = -5.0


def of_module_inputs(pix_trans, nb=NB, nf=NF, held=False):
    """The script's per-frame random inputs (of_module.py:111,122) and its pixel coordinates.  held: step HELD_STEP's control is
    HELD_CONTROL on every axis and the next step's takes it back, so that step - and only that - finds <= 3 feasible points."""
    rng = np.random.default_rng(77)
    controls = rng.normal(0, 0.01, (nf - 1, nb, 3)); omegas = rng.normal(0, 0.01, (nf - 1, nb, 3))
    if held:
        controls[HELD_STEP - 1] = HELD_CONTROL; controls[HELD_STEP] = -HELD_CONTROL
    cx, cy = pix_trans((H, W))
    return dict(controls=controls, omegas=omegas, cx=cx, cy=cy, normal=np.array([0.0, 0.0, 1.0]))


def of_module_cfg(PipelineConfig, zones=True, grid=OFM_GRID):
    cfg = PipelineConfig.of_module()
    for k, v in OFM.items():
        setattr(cfg, k, v)
    if zones:
        cfg.zones, cfg.zone_link, cfg.zone_min = "hull", OFM_ZONES["link"], OFM_ZONES["min_members"]
    if grid:
        cfg.grid_cell, cfg.grid_cap, cfg.grid_max_rank = grid
    return cfg


def of_module_reference(frames_b, cfg, inp, b, model, hold=False, grid_log=None, zones=OFM_ZONES, age_on_hold=False):
    """oracle_of_module of stream b with the zone table and, when cfg has one, the grid.  age_on_hold: the deliberately wrong
    reference of the held-step test's self-check - the table ages on a held step too."""
    detect = cg.grid_detect(cfg, grid_of(cfg), grid_log) if cfg.grid_cell else None
    first, steps = oracle_of_module(frames_b, cfg, inp["normal"], inp["controls"][:, b], inp["omegas"][:, b], OFM_MIN_FEAT, inp["cx"], inp["cy"], model,
                                    False, hold=hold, detect=detect, zones=zones)
    if age_on_hold:
        steps = _aged_on_hold(steps)
    return first, steps


def _aged_on_hold(steps):
    """The steps' tables as a loop that ran rule 7 on held steps too would report them.  Only the held steps themselves are rewritten
    (what follows would differ as well; the first difference is what the self-check needs)."""
    import zones_reference as zr
    out = []
    for s in steps:
        if s[6]["held"]:
            t = s[6]["zones"].copy()
            zr.age(t)
            s = s[:6] + (dict(s[6], zones=t),)
        out.append(s)
    return out


# ---------------------------------------------------------------------------------------- frame pairs
PAIR_CFG = dict(BASE, **SEED, **GATE, **GRID, **ROBUST, **COV)
PAIR_FRAMES = ((0, 0), (1, 0), (0, 3))                           # (stream, frame t): the pair t -> t + 1; three pairs straddle two slices


def pair_frames(frames):
    return np.stack([frames[b, t] for b, t in PAIR_FRAMES]), np.stack([frames[b, t + 1] for b, t in PAIR_FRAMES])


def pair_references(cfg, prev, nxt, sr, predict=None):
    """batch_oracle.combined_chain of every pair, held to the robust comparison's conditions (no near-tie: no allowance needed)."""
    from batch_oracle import combined_chain
    mode = ls.SEED_MODEL if cfg.lk_seed == "model" else ls.SEED_ROTATION
    refs = [combined_chain(prev[b], nxt[b], cfg, sr[b], b, grid_of(cfg), gate_of(cfg), mode, dict(rso.SETTING), cov_dict(cfg), cfg.seed_gain, predict)
            for b in range(len(prev))]
    for b, r in enumerate(refs):
        assert r["robust"]["gap"] >= 1e-6 and r["robust"]["near"] == 0, (b, r["robust"]["gap"], r["robust"]["near"])
    return refs
