"""The frame pairs, stream sequences and settings of tests/test_gpu_rs.py, which tests/test_gpu_finite.py runs the finite motion on as
well: one scene, two test files.  No test file."""
import numpy as np

import camera_reference as CR
import cov_reference as cr

H, W, B, CORNERS = 120, 160, 4, 48
F = 160.0
MOTION = dict(v=(0.02, -0.03, 0.01), omega=(0.004, -0.003, 0.004), d=1.0)
PAIR_CAM = dict(fx=F, fy=F, cx=80.0, cy=60.0, k=CR.STRONG[1])
_cache = {}


def as_struct(ofk, rs):
    """rs_reference's dict -> ofk.RShutter, field by field (no defaults in between)."""
    return ofk.RShutter(rs["mode"], rs["rows"], rs["readout"], rs["anchor"], rs["omega_gain"])


# ---------------------------------------------------------------------------------------------------- frame pairs
def pair_batch(pkg, ofk):
    if "pairs" not in _cache:
        from of_amd import synth
        prev, nxt, base = synth.make_batch(B, H, W, seed=5100, distinct=B, margin=64, scaling=1.0 / F, **MOTION)
        sensors = ofk.make_sensors(B, d=MOTION["d"], normal=base[0]["n"], omega=MOTION["omega"], offset=(0.02, -0.01, 0.2), scaling=1.0 / F,
                                   cx=W / 2.0, cy=H / 2.0, v_prior=MOTION["v"])
        _cache["pairs"] = (prev, nxt, sensors)
    return _cache["pairs"]


def pair_cfg(**kw):
    from of_amd.pipeline import PipelineConfig
    return PipelineConfig(max_corners=CORNERS, quality=0.01, min_distance=6, block_size=7, win=15, max_level=2, max_count=20, eps=0.03, **kw)


COVD = dict(mode=cr.PROPAGATE, sigma_flow=0.3, sigma_pos=0.5, sigma_d=0.04, sigma_omega=(0.01, 0.02, 0.015), sigma_normal=0.004, sigma_offset=0.006,
            filter_r=False, r_floor=0.0, nis_max=0.0, omega_from_imu=False)
COV = dict(cov="propagate", sigma_flow_px=0.3, sigma_pos_px=0.5, sigma_d=0.04, sigma_omega=(0.01, 0.02, 0.015), sigma_normal=0.004, sigma_offset=0.006)
GATE = dict(fb_check="seeded", fb_thr=0.05, fb_level=0, err_max=6.0)
SEED = dict(lk_seed="model", seed_gain=1.0)


# ---------------------------------------------------------------------------------------------------- streams
SH, SW, NB, NSTEPS, S_CORNERS, MIN_FEAT, RADIUS, FEAS_T = 96, 128, 2, 4, 40, 39, 8, 0.04
S_MOTION = dict(v=(0.02, -0.03, 0.004), omega=(0.004, -0.003, 0.008), d=1.0)


def stream_setup(pkg, ofk, kind):
    from of_amd import synth
    from of_amd.pipeline import PipelineConfig
    if "seq" not in _cache:
        seqs = [synth.render_sequence(SH, SW, 6100 + b, NSTEPS + 1, scaling=1.0 / SW, margin=64, **S_MOTION) for b in range(NB)]
        _cache["seq"] = (np.stack([s[0] for s in seqs]), seqs[0][1])
    frames, info = _cache["seq"]
    sensors = ofk.make_sensors(NB, d=info["d"], normal=info["n"], omega=info["omega"], offset=(0.02, -0.01, 0.2), scaling=info["scaling"], cx=info["cx"],
                               cy=info["cy"], v_prior=info["v"])
    cfg = PipelineConfig(max_corners=S_CORNERS, quality=0.01, min_distance=6, block_size=7, win=15, max_level=2, max_count=20, eps=0.03, zones="hull",
                         **({} if kind == "step" else dict(use_feasibility=True, feas_T=FEAS_T)))
    return frames, sensors, cfg
