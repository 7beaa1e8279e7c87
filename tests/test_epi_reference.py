"""CPU-only: the epipolar solve of ofk.h (ofk_set_epipolar) as tests/epi_reference.py restates it - against an independent route, on
exact flow over arbitrary depths, at its flags, under finite motion, and on the experiment that motivates it.

TOL, the tolerance the GPU tests hold the device to as well, is pinned here: 16 x the largest relative deviation of (t^, s) between
the restatement (the kernel's summation order, N0^(-1/2) from an eigen-decomposition) and the independent route (plain sums, a
Cholesky factor of N0, eigh on the whitened matrix, np.linalg.lstsq for s) over every case below (the convention of
tests/test_joint_reference.py).  Measured: MEASURED_DEV below.

The experiment (epi_reference.scene: 400 points over 1280 x 960, f = 1000, range 1.5 along the optical axis, v = (0.02, -0.015, 0.004)
and omega = (0.004, -0.003, 0.01) per frame, 0.2 px of flow noise; the ground inside 0.12 of the beam's foot level, the rest carrying
relief h with Z = Z_plane (1 - h); anchor 0.12), median relative error of v over the seeds 0-19, measured with the committed code:
    scene                                      plain    robust (Tukey, K = 64)   epipolar   t^ off by   rho_i off by (median)
    block of 0.3 on 30 % of the frame          0.2240   0.0018                   0.0025     0.080 deg   0.74 %
    the same block on 60 %                     0.3094   0.4284                   0.0024     0.082 deg   0.68 %
    canopy, 60 % raised by 0.1 .. 0.5          0.2654   0.2460                   0.0017     0.048 deg   0.67 %
    ramp rising to 0.35 across the frame       0.2726   0.2738                   0.0025     0.080 deg   0.69 %
The figures of the covariance grid and the gate's default are in test_covariance_grid_and_the_gate_default's docstring, those of the
rendered pair in test_rendered_pair_through_the_oracle_chain's."""
import hashlib

import numpy as np
import pytest

import epi_reference as er
import finite_reference as fr
import robust_reference as rr

MEASURED_DEV = 6.9e-16                                          # 65 points, NODE, unit weights
TOL = 16 * MEASURED_DEV
MEASURED = dict(dev=0.0)
EPI_SIGMA_MAX = 0.008                                           # the default of epi_sigma_max, derived in the grid test below


def case(n, weights):
    """The scene of count n: relief with the anchor at the foot from 8 points on; below that level ground and every point an anchor."""
    x, u, d, nrm, om, v, rho = er.scene(n, 1000 + n, kind="canopy" if n >= 8 else "flat", outliers=weights)
    kw = dict(anchor=er.FOOT, anchor_min=5) if n >= 8 else dict(anchor=np.inf, anchor_min=1)
    w = er.robust_weights(x, u, d, nrm, om) if weights else None
    return x, u, d, nrm, om, v, rho, w, kw


def deviation(n, variant, weights):
    x, u, d, nrm, om, v, rho, w, kw = case(n, weights)
    if weights and n >= 64:
        assert np.any((w > 0) & (w < 1))                         # real weights, not all ones
    vs, rss, _ = er.plain_solve(variant, x, u, d, nrm, om, None, w)
    got = er.epi_solve(x, u, d, nrm, om, weights=er.W_ROBUST if weights else er.W_ONE, w=w, v_s=vs, rss_s=rss, **kw)
    assert got["flag"] == 0 and got["rewritten"], (n, variant, weights, got["flag"])
    ti, si = er.epi_independent(x, u, d, nrm, om, anchor=kw["anchor"], w=w, weights=er.W_ROBUST if weights else er.W_ONE)
    return er.rel_dev(got["t"], got["s"], ti, si)


@pytest.mark.parametrize("n", er.COUNTS)
def test_restatement_against_the_independent_route(n):
    for variant in (er.NODE, er.SIM):
        for weights in (False, True):
            dev = deviation(n, variant, weights)
            if dev > MEASURED["dev"]:
                MEASURED.update(dev=dev, at=(n, variant, weights))
            assert dev <= TOL, (n, variant, weights, dev)
    print(f"n {n}: largest relative deviation of (t^, s) so far {MEASURED['dev']:.3e} at {MEASURED.get('at')}")


def test_exact_flow_over_arbitrary_depths_returns_the_truth():
    for n in (8, 65, 400):
        x, u, d, nrm, om, v, rho = er.scene(n, 7 + n, kind="canopy", noise=0.0)
        rng = np.random.default_rng(n)
        out = np.hypot(x[:, 0], x[:, 1]) > er.FOOT
        rho = np.where(out, rho * rng.uniform(0.5, 2.0, n), rho)  # depths that follow no surface at all
        u = er.flow(x, v, om, rho)
        got = er.epi_solve(x, u, d, nrm, om, anchor=er.FOOT)
        assert got["flag"] == 0
        assert np.abs(got["v"] - v).max() <= 1e-11 * np.linalg.norm(v), (n, got["v"] - v)
        assert np.abs(got["rho"] / rho - 1.0).max() <= 1e-11, n
        assert got["rec"][16] <= 1e-24 * got["rec"][14] and got["rec"][4] <= 1e-12 * er.SIGMA_FLOW
        assert np.all(got["rows"][:, 3] == 0) and got["rec"][13] == 0
        plain = er.plain_solve(er.NODE, x, u, d, nrm, om)[0]
        assert np.linalg.norm(plain - v) / np.linalg.norm(v) > 0.05       # what the one plane costs the plain solve here


KINDS = ("block30", "block60", "canopy", "ramp")
# recorded with the committed code (the module docstring's table): plain, robust, epipolar
RECORDED = {"block30": (0.2240, 0.0018, 0.0025), "block60": (0.3094, 0.4284, 0.0024), "canopy": (0.2654, 0.2460, 0.0017),
            "ramp": (0.2726, 0.2738, 0.0025)}


def experiment(kind, seeds=range(20)):
    rows = []
    for seed in seeds:
        x, u, d, nrm, om, v, rho = er.scene(400, seed, kind)
        nv = np.linalg.norm(v)
        plain = er.plain_solve(er.NODE, x, u, d, nrm, om)[0]
        rob = rr.robust_solve(rr.NODE, x, u, d, nrm, om, loss=rr.TUKEY, hypotheses=64, seed=seed)["v"]
        got = er.epi_solve(x, u, d, nrm, om, anchor=er.FOOT, fast=True)
        assert got["flag"] == 0, (kind, seed)
        rows.append((np.linalg.norm(plain - v) / nv, np.linalg.norm(rob - v) / nv, np.linalg.norm(got["v"] - v) / nv,
                     np.degrees(np.arccos(min(1.0, got["t"] @ v / nv))), np.median(np.abs(got["rho"] / rho - 1.0))))
    return np.median(np.array(rows), 0)


@pytest.mark.parametrize("kind", KINDS)
def test_relief_experiment(kind):
    plain, rob, epi, ang, drho = experiment(kind)
    print(f"{kind}: plain {plain:.4f}  robust {rob:.4f}  epipolar {epi:.4f}  t^ off by {ang:.3f} deg  rho off by {100 * drho:.2f} %")
    assert epi < plain / 10, (kind, plain, epi)
    if kind != "block30":
        assert epi < rob / 10, (kind, rob, epi)
    assert epi <= 3 * RECORDED[kind][2] and plain >= RECORDED[kind][0] / 3


SPEEDS = (0.0005, 0.001, 0.002, 0.004, 0.008, 0.016, 0.025)
DIRECTIONS = {"lateral": (1.0, 0.0, 0.0), "diagonal": (0.8, -0.6, 0.16), "forward": (0.3, 0.2, 1.0)}
GRID_COUNTS = (50, 400)


def covariance_grid(seeds=40):
    """[(count, direction, speed, predicted rms 1 sigma, measured rms angle, mean sigma^ / sigma)] over canopy scenes, every kept
    point an anchor (the scale does not enter the direction)."""
    rows = []
    for n in GRID_COUNTS:
        for name, dv in DIRECTIONS.items():
            dv = np.asarray(dv) / np.linalg.norm(dv)
            for sp in SPEEDS:
                ang, pred, sig = [], [], []
                for seed in range(seeds):
                    x, u, d, nrm, om, v, rho = er.scene(n, seed, "canopy", v=sp * dv)
                    got = er.epi_solve(x, u, d, nrm, om, anchor=np.inf, anchor_min=1, fast=True)
                    assert got["flag"] == 0
                    ang.append(np.arccos(min(1.0, abs(got["t"] @ dv)))); pred.append(got["pred"]); sig.append(got["sigma"])
                rows.append((n, name, sp, float(np.sqrt(np.mean(np.square(pred)))), float(np.sqrt(np.mean(np.square(ang)))),
                             float(np.mean(sig)) / er.SIGMA_FLOW))
    return rows


def test_covariance_grid_and_the_gate_default(pkg):
    """Measured / predicted rms direction error (40 seeds per cell, canopy relief, 0.2 px of noise), by speed |v| per frame at range
    1.5 (f = 1000: 0.0005 is a third of a pixel of flow, 0.025 is 17 px).  Each cell: predicted 1 sigma in rad / ratio.
        count direction  0.0005      0.001       0.002       0.004       0.008       0.016       0.025
        50    lateral    0.164/2.52  0.115/1.43  0.062/1.13  0.032/1.04  0.016/1.01  0.008/1.00  0.005/0.99
        50    diagonal   0.169/1.57  0.104/1.02  0.054/0.89  0.028/0.86  0.014/0.85  0.007/0.84  0.004/0.84
        50    forward    0.080/5.21  0.041/2.71  0.028/1.63  0.016/1.38  0.008/1.30  0.004/1.27  0.003/1.27
        400   lateral    0.068/1.61  0.040/1.02  0.021/0.89  0.011/0.87  0.005/0.86  0.003/0.87  0.002/0.87
        400   diagonal   0.063/1.20  0.036/0.91  0.019/0.86  0.010/0.86  0.005/0.86  0.002/0.86  0.002/0.87
        400   forward    0.016/5.04  0.013/2.28  0.009/1.55  0.005/1.32  0.003/1.26  0.001/1.24  0.001/1.24
    sigma^ / sigma is 0.93 - 1.01 throughout (0.97 - 1.01 from 0.001 on).
    Sorted by prediction, the first cell whose ratio reaches 1.5 is the forward motion of 0.002 at 400 points, predicted 0.0092 rad;
    the largest prediction below it is 0.0081 rad.  Lateral and diagonal motion alone would allow 0.06 rad; motion along the optical
    axis puts the epipole inside the frame, where |b_i| is small and the first-order prediction gives out earlier.  The default of
    epi_sigma_max is therefore 0.008 rad: every cell of the grid predicted below it has a ratio under 1.5."""
    from of_amd import ofk
    from of_amd.pipeline import PipelineConfig
    rows = sorted(covariance_grid(), key=lambda r: r[3])
    for n, name, sp, pred, rms, sg in rows:
        print(f"{n:4d} {name:9s} {sp:7.4f}  predicted {pred:.4f}  measured {rms:.4f}  ratio {rms / pred:5.2f}  sigma^/sigma {sg:.2f}")
    bad = [r for r in rows if r[4] / r[3] >= 1.5]
    limit = max(r[3] for r in rows if r[3] < bad[0][3])          # the largest prediction up to which the ratio stays below 1.5
    print(f"ratio below 1.5 up to a prediction of {limit:.4f} rad; first miss at {bad[0][3]:.4f} ({bad[0][:3]})")
    assert ofk.EPI_SIGMA_MAX == PipelineConfig().epi_sigma_max == ofk.epipolar_setting().sigma_max == EPI_SIGMA_MAX
    assert EPI_SIGMA_MAX <= limit < 1.25 * EPI_SIGMA_MAX          # the default is that limit, rounded down
    inside = [r for r in rows if r[3] <= EPI_SIGMA_MAX]
    assert len(inside) >= 12 and all(0.7 <= r[4] / r[3] < 1.5 for r in inside)
    assert all(0.9 <= r[5] <= 1.1 for r in rows)                 # the flow noise comes back from the constraint alone


def test_flags():
    x, u, d, nrm, om, v, rho = er.scene(65, 6)
    kw = dict(anchor=er.FOOT)
    ok = er.epi_solve(x, u, d, nrm, om, **kw)
    assert ok["flag"] == 0 and ok["rec"][10] == 0.0 and ok["rec"][11] == 65 and ok["rec"][12] >= 5
    vs = ok["rec"][6:9]
    for few in (1, 2):                                           # flag 1: one or two points
        g = er.epi_solve(x[:few], u[:few], d, nrm, om, anchor=np.inf, anchor_min=1)
        assert g["flag"] == 1 and g["rec"][10] == 1.0 and g["rec"][11] == few and not g["rewritten"] and not g["rows"].any()
        assert np.all(np.delete(g["rec"], [6, 7, 8, 9, 10, 11]) == 0)
    for bad_d in (0.0, np.nan, np.inf):                          # d0 = 0, a NaN range
        g = er.epi_solve(x, u, bad_d, nrm, om, v_s=vs, rss_s=0.0, **kw)
        assert g["flag"] == 1 and np.array_equal(g["v"], vs) and not g["rows"].any(), bad_d
    xn = x.copy(); xn[7, 0] = np.nan
    assert er.epi_solve(xn, u, d, nrm, om, v_s=vs, rss_s=0.0, **kw)["flag"] == 1
    assert er.epi_solve(x, u, d, nrm, om, beam=(1.0, 0.0, 0.0), v_s=vs, rss_s=0.0, **kw)["flag"] == 1       # e_z == 0
    assert er.epi_solve(x, u, d, (1.0, 0.0, 0.0), om, v_s=vs, rss_s=0.0, **kw)["flag"] == 1                 # n0.e == 0
    # flag 2: a hover - the direction is noise, the prediction says so
    xh, uh, *_ = er.scene(65, 6, v=(0.0, 0.0, 0.0))
    g = er.epi_solve(xh, uh, d, nrm, om, sigma_max=EPI_SIGMA_MAX, **kw)
    assert g["flag"] == 2 and g["rec"][10] == 2.0 and g["pred"] > EPI_SIGMA_MAX and not g["rewritten"] and not g["rows"].any()
    assert g["rec"][3] == 0 and np.all(g["rec"][18:31] == 0) and g["rec"][17] == g["pred"] and abs(np.linalg.norm(g["rec"][0:3]) - 1) < 1e-12
    assert er.epi_solve(xh, uh, d, nrm, om, sigma_max=np.inf, **kw)["flag"] in (0, 3)                       # the gate alone stops it
    # flag 3: an empty anchor; anchor_min not met
    g = er.epi_solve(x, u, d, nrm, om, anchor=1e-6)
    assert g["flag"] == 3 and g["rec"][12] == 0 and g["rec"][3] == 0 and np.all(g["rec"][24:31] == 0) and np.any(g["rec"][18:24] != 0)
    assert not g["rewritten"] and np.array_equal(g["v"], g["rec"][6:9]) and not g["rows"].any()
    na = int(ok["rec"][12])
    assert er.epi_solve(x, u, d, nrm, om, anchor=er.FOOT, anchor_min=na)["flag"] == 0
    assert er.epi_solve(x, u, d, nrm, om, anchor=er.FOOT, anchor_min=na + 1)["flag"] == 3


def test_sign_flip_and_a_point_behind_the_camera():
    x, u, d, nrm, om, v, rho = er.scene(257, 9)
    g = er.epi_solve(x, u, d, nrm, om, anchor=er.FOOT)             # whichever eigenvector the decomposition returns, t^ points along v
    assert g["flag"] == 0 and g["t"] @ v > 0 and g["s"] > 0 and np.all(g["rho"] > 0)
    # the mirrored motion: same lines, opposite direction - the sign rule follows the flow, not the decomposition
    um = er.flow(x, -v, om, rho)
    g = er.epi_solve(x, um, d, nrm, om, anchor=er.FOOT)
    assert g["flag"] == 0 and g["t"] @ v < 0 and np.abs(g["v"] + v).max() <= 1e-11 and np.all(g["rho"] > 0)
    # one point whose flow runs against the rest: kappa <= 0, point flag 2, counted in slot 13
    u2 = u.copy()
    u2[100] = er.flow(x[100:101], v, om, -rho[100:101])[0]
    g = er.epi_solve(x, u2, d, nrm, om, anchor=er.FOOT)
    assert g["flag"] == 0 and g["rec"][13] == 1 and g["rows"][100, 3] == 2.0 and g["rows"][100, 0] < 0
    assert np.all(np.delete(g["rows"][:, 3], 100) == 0)
    valid = np.ones(257, np.uint8); valid[[3, 50]] = 0
    g = er.epi_solve(x, u, d, nrm, om, anchor=er.FOOT, valid=valid)
    assert g["flag"] == 0 and g["rec"][11] == 255 and np.array_equal(np.flatnonzero(g["rows"][:, 3] == 1), [3, 50]) and not g["rows"][[3, 50], :3].any()


def test_finite_motion_constraint_is_exact_whatever_the_depths():
    """The rewritten points of tests/finite_reference.py at 156 px of flow: c = x^ x u^ is parallel to q~ x p1 whatever the plane
    factor s in u^, so c.T = 0 to rounding for points at ANY depth, and on the plane itself v = T."""
    m = fr.MOTIONS[3]
    sc = fr.exact_scene(m["T"], m["omega"])
    sr = fr.sensor_row(sc)
    assert fr.max_flow_px(sc, sr) > 150
    T = np.asarray(m["T"]); om = np.asarray(m["omega"])
    # the plane's own points
    o0, o1, good = fr.correct_f64(fr.setting(), fr.to_px(sc["x0"], sr), fr.to_px(sc["x1"], sr), sr)
    assert good.all()
    x, u = fr.xu(o0, o1, sr)
    g = er.epi_solve(x, u, sr[0], sr[1:4], om, anchor=np.inf)
    assert g["flag"] == 0 and np.abs(g["v"] - T).max() <= 1e-11 * np.linalg.norm(T) and g["rec"][16] <= 1e-24 * g["rec"][14]
    raw = er.epi_solve(*fr.xu(fr.to_px(sc["x0"], sr), fr.to_px(sc["x1"], sr), sr), sr[0], sr[1:4], om, anchor=np.inf)
    assert np.linalg.norm(raw["v"] - T) / np.linalg.norm(T) > 0.01          # the raw points at this flow are no instantaneous field
    # points at depths the sensors' plane knows nothing of
    rng = np.random.default_rng(4)
    p0 = np.concatenate([sc["x0"], np.ones((len(sc["x0"]), 1))], 1)
    P0 = p0 * rng.uniform(0.6, 3.0, len(p0))[:, None]
    P1 = P0 @ sc["R"].T + T
    x1 = P1[:, :2] / P1[:, 2:3]
    o0, o1, good = fr.correct_f64(fr.setting(), fr.to_px(sc["x0"], sr), fr.to_px(x1, sr), sr)
    x, u = fr.xu(o0[good], o1[good], sr)
    assert good.sum() > 300
    p = np.concatenate([x, np.ones((len(x), 1))], 1)
    c = np.cross(p, np.concatenate([u, np.zeros((len(x), 1))], 1) + np.cross(p, om[None, :]))
    worst = np.abs(c @ T).max() / (np.linalg.norm(c, axis=1).max() * np.linalg.norm(T))
    print(f"finite motion, arbitrary depths: largest |c.T| / (|c| |T|) {worst:.2e}")
    assert worst <= 1e-14
    g = er.epi_solve(x, u, sr[0], sr[1:4], om, anchor=np.inf, anchor_min=1)
    assert g["flag"] == 0 and np.linalg.norm(np.cross(g["t"], T / np.linalg.norm(T))) <= 1e-12


LINEAR_SHA256 = "9acc4d3299baf8e8996edaa9aa68c89bb5223f3d46b33d2f37e739f35ad888bf"      # render_pair(48, 64, 3) before the option existed
RENDER = dict(h=480, w=640, v=(0.02, -0.015, 0.004), omega=(0.004, -0.003, 0.01), d=1.5, rect=(420, 0, 640, 480), height=0.3, anchor_px=90.0)
RENDER_SEEDS = (20, 21, 22, 23)


def rendered_pair(synth, seed):
    r = RENDER
    return synth.render_pair(r["h"], r["w"], seed, margin=96, v=r["v"], omega=r["omega"], d=r["d"], relief=dict(rect=r["rect"], height=r["height"]))


def test_render_pair_relief(pkg):
    from of_amd import synth
    r = synth.render_pair(48, 64, 3)
    assert hashlib.sha256(r["prev"].tobytes() + r["next"].tobytes() + r["H"].tobytes()).hexdigest() == LINEAR_SHA256
    n = synth.render_pair(48, 64, 3, relief=None)
    assert all(np.array_equal(r[k], n[k]) for k in ("prev", "next", "H")) and sorted(r) == sorted(n)
    p = synth.render_pair(48, 64, 3, v=(0.03, 0.0, 0.0), omega=(0.0, 0.0, 0.0), relief=dict(rect=(32, 8, 60, 40), height=0.4))
    q = synth.render_pair(48, 64, 3, v=(0.03, 0.0, 0.0), omega=(0.0, 0.0, 0.0))
    assert np.array_equal(p["prev"], q["prev"]) and np.array_equal(p["H"], q["H"])
    diff = np.any(p["next"] != q["next"], -1)
    assert diff[8:40, 32:60].mean() > 0.5 and not diff[:8].any() and not diff[40:].any() and not diff[:, :32].any() and not diff[:, 60:].any()
    # the raised plane moves faster by 1 / (1 - h)
    assert np.allclose((p["H_relief"] - np.eye(3))[0, 2], (q["H"] - np.eye(3))[0, 2] / 0.6, rtol=1e-12)
    from of_amd.pipeline import RollingShutter
    with pytest.raises(ValueError):
        synth.render_pair(48, 64, 3, relief=dict(rect=(0, 0, 8, 8), height=0.2), rolling_shutter=RollingShutter(readout=0.5))
    with pytest.raises(ValueError):
        synth.render_pair(48, 64, 3, relief=dict(rect=(0, 0, 80, 8), height=0.2))


def rendered(synth, PipelineConfig, io):
    import lk_seed_reference as lr
    cfg = PipelineConfig(max_corners=300, quality=0.01, min_distance=10, block_size=7, win=15, max_level=3, max_count=20, eps=0.03)
    rows = []
    for seed in RENDER_SEEDS:
        pair = rendered_pair(synth, seed)
        g0, g1 = io.gray_bgr8(pair["prev"]), io.gray_bgr8(pair["next"])
        pts = io.good_features(g0, cfg.max_corners, cfg.quality, cfg.min_distance, cfg.block_size)
        sr = lr.experiment_sensors(pair)
        seedpts = lr.predict(pts.reshape(-1, 2), sr).reshape(pts.shape)
        n, s, e = lr.lk_pyr(g0, g1, pts, cfg.win, cfg.max_level, cfg.max_count, cfg.eps, cfg.min_eig_thr, seed=seedpts, flags=4)
        ok = s.ravel() == 1
        new = n.reshape(-1, 2).astype(np.float64); old = pts.reshape(-1, 2).astype(np.float64)
        x = (new - [pair["cx"], pair["cy"]]) * pair["scaling"]; u = (new - old) * pair["scaling"]
        truth = pair["v"]
        plain = er.plain_solve(er.NODE, x, u, pair["d"], pair["n"], pair["omega"], ok)[0]
        rob = rr.robust_solve(rr.NODE, x, u, pair["d"], pair["n"], pair["omega"], valid=ok, loss=rr.TUKEY, hypotheses=64, seed=seed)["v"]
        got = er.epi_solve(x, u, pair["d"], pair["n"], pair["omega"], anchor=RENDER["anchor_px"] * pair["scaling"], sigma_max=np.inf, valid=ok)
        on_roof = new[:, 0] >= RENDER["rect"][0]
        rho_true = np.where(on_roof, 1.0 / (1.0 - RENDER["height"]), 1.0) / pair["d"]
        used = got["rows"][:, 3] == 0
        drho = np.median(np.abs(got["rows"][used & ok, 0] / rho_true[used & ok] - 1.0)) if got["flag"] == 0 else np.nan
        nv = np.linalg.norm(truth)
        rows.append((seed, int(ok.sum()), np.linalg.norm(plain - truth) / nv, np.linalg.norm(rob - truth) / nv, np.linalg.norm(got["v"] - truth) / nv,
                     got["flag"], got["rec"][12], got["sigma"] / pair["scaling"], got["pred"], drho))
    return rows


def test_rendered_pair_through_the_oracle_chain(pkg):
    """A rendered 480 x 640 pair whose right third is a roof of height 0.3 (RENDER), corners of the C oracle, LK seeded from the sensor
    model as the finite-motion scene seeds it; the anchor is 90 px around the image centre.
    Recorded with the committed code (seed: tracked points, relative error of v plain, robust, epipolar; anchors, sigma^ in px,
    predicted 1 sigma of the direction, median error of rho_i):
        20: 300   0.3124   0.0112   0.0133   25   0.228   0.0043   0.10 %
        21: 299   0.3250   0.0110   0.0241   27   0.394   0.0080   0.34 %
        22: 294   0.3056   0.0112   0.0147   19   0.389   0.0076   0.12 %
        23: 295   0.2839   0.0112   0.0162   34   0.283   0.0053   0.29 %
    With one roof on a third of the frame the ground still holds the majority, so the robust solve does as well here (the 60 % block,
    the canopy and the ramp of the experiment above are where it cannot).  The tracker's errors along the roof's edge lift sigma^ to
    0.4 px; seed 21's prediction then sits at the default gate (0.0080 rad), so the gate is left open here and the figure printed.
    Asserted: flag 0, plain > 0.05, epipolar < plain / 4."""
    from of_amd import synth
    from of_amd.pipeline import PipelineConfig
    from oracle import image_oracle as io
    for seed, m, plain, rob, epi, flag, na, sig, pred, drho in rendered(synth, PipelineConfig, io):
        print(f"seed {seed}: {m} points, plain {plain:.4f}, robust {rob:.4f}, epipolar {epi:.4f}, flag {flag}, {int(na)} anchors, "
              f"sigma^ {sig:.3f} px, predicted {pred:.4f} rad, rho off by {100 * drho:.2f} %")
        assert flag == 0
        assert plain > 0.05 and epi < plain / 4, (seed, plain, epi)


def test_pair_epi_behind_an_unsolved_step():
    """solved=False (a stream step whose record[15] is 0): flag 1 in the header's layout - everything but slots 6-11 is 0, every point
    row is 0 - and v / rss are the record's own; the same points with solved=True solve."""
    from test_joint_reference import pixel_points, sensor_row
    x, u, d, nrm, om, v, rho = er.scene(65, 1065)
    sr = sensor_row(d, nrm, om)
    prev, nxt = pixel_points(x, u, sr)
    status = np.ones(65, np.uint8); status[10::9] = 0
    for rec in (np.zeros(16), np.concatenate([[0.01, -0.02, 0.003, 4e-7, 3.0], np.zeros(11)])):
        got = er.pair_epi(prev, nxt, status, sr, rec, anchor_px=120.0, solved=False)
        r = got["rec"]
        assert got["flag"] == 1 and r[10] == 1.0 and not got["rewritten"] and np.array_equal(got["v"], rec[0:3]) and got["rss"] == rec[3]
        assert np.array_equal(r[6:10], rec[0:4]) and r[11] == np.count_nonzero(status) and not np.delete(r, [6, 7, 8, 9, 10, 11]).any()
        assert got["rows"].shape == (65, 4) and not got["rows"].any()
    on = er.pair_epi(prev, nxt, status, sr, rec, anchor_px=120.0, solved=True)
    assert on["flag"] == 0 and on["rewritten"] and on["rows"][status == 0, 3].all()
