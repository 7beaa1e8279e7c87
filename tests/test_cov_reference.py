"""CPU-only: pins tests/cov_reference.py, the numpy reference the device covariance is compared with.

  * every Jacobian block against central differences (h = 1e-6) of the oracle's solve_lgs_node / _sim / _eval, to 1e-6 of the block's
    largest entry (the difference quotient's own noise here is ~1e-9; the figures are printed); v is exactly linear in u, omega and d
    for fixed points, so those blocks also satisfy J delta = Delta v for a finite delta to 1e-10;
  * residual mode = sigma^2 inv(A^T A) with A stacked as the oracle stacks it;
  * the reference's own recorded Monte-Carlo sweeps (tests/golden/reference_sweeps.npz): recorded / predicted standard deviation, rms
    over steps 1..99, within [0.80, 1.25] per component, and at most 2 % of the single-step ratios outside +-35 %.  Each stored value
    is an estimate from 100 unseeded trials (+-7 % per step), so the bounds keep a wrong term from hiding; they are not fits;
  * structure: symmetric, positive semi-definite, shares sum to the trace, doubling a sigma quadruples exactly its share, filter_r
    with a void covariance is the constant-R filter."""
import os

import numpy as np
import pytest

import cov_reference as cr
from oracle import estimation_oracle as eo

HERE = os.path.dirname(os.path.abspath(__file__))
TRUTH = dict(v=np.array([1.0, 1, 1]), omega=np.array([1.0, 1, 1]), d=1.0, n=np.array([0.0, 0, 1]), t=np.array([0.02, 0, 0.205]))


@pytest.fixture(scope="module")
def sweeps():
    return np.load(os.path.join(HERE, "golden", "reference_sweeps.npz"))


def centred(raw):
    d = np.array(raw, np.float64)[:, :2].copy()
    d[:, 0] = (d[:, 0] - np.mean(d[:, 0])) * 1.27; d[:, 1] = (d[:, 1] - np.mean(d[:, 1])) * 0.93
    return d


def scene12():
    rng = np.random.default_rng(12)
    x = rng.uniform(-0.6, 0.6, (12, 2))
    n = np.array([0.05, -0.08, 1.0]); n /= np.linalg.norm(n)
    om = np.array([0.1, -0.2, 0.15]); v = np.array([0.4, -0.3, 0.2]); d = 2.5; t = np.array([0.02, -0.01, 0.2])
    u = eo.generate_test_data(x, v, om, d, n) + rng.normal(0, 1e-3, (12, 2))      # not an exact fit: the residual terms matter
    return x, u, d, n, om, t


def scenes(sweeps):
    x = centred(sweeps["points_raw"])
    T = TRUTH
    u = eo.generate_test_data(x, T["v"], T["omega"], T["d"], T["n"], T["t"])
    return {"points200": (x, u, T["d"], T["n"], T["omega"], T["t"]), "scene12": scene12()}


SOLVERS = {
    "node": (cr.NODE, False, lambda x, u, d, n, om, t: eo.solve_lgs_node(x, u, d, n, om)[0]),
    "sim": (cr.SIM, True, lambda x, u, d, n, om, t: eo.solve_lgs_sim(x, u, d, n, om, t)[0]),
    "eval": (cr.NODE, True, lambda x, u, d, n, om, t: eo.solve_lgs_eval(x, u, d, n, om, t)[0]),
}


def central(f, args, which, idx, h=1e-6):
    a = [np.array(v, np.float64) for v in args]
    lo = [v.copy() for v in a]; hi = [v.copy() for v in a]
    if a[which].ndim == 0:
        lo[which] = a[which] - h; hi[which] = a[which] + h
    else:
        lo[which][idx] -= h; hi[which][idx] += h
    return (f(*hi) - f(*lo)) / (2 * h)


@pytest.mark.parametrize("scene", ["points200", "scene12"])
@pytest.mark.parametrize("solver", ["node", "sim", "eval"])
def test_jacobian_blocks_against_central_differences(sweeps, scene, solver):
    x, u, d, n, om, t = scenes(sweeps)[scene]
    variant, lever, f = SOLVERS[solver]
    args = (x, u, d, n, om, t)
    J = cr.jacobians(variant, x, u, d, n, om, t=t if lever else None)
    N = len(x)
    pts = sorted(set([0, 1, N // 2, N - 1]))
    blocks = {
        "Ju": (J["Ju"][:, pts, :], np.stack([np.stack([central(f, args, 1, (i, c)) for c in range(2)], 1) for i in pts], 1)),
        "Jx": (J["Jx"][:, pts, :], np.stack([np.stack([central(f, args, 0, (i, c)) for c in range(2)], 1) for i in pts], 1)),
        "Jw": (J["Jw"], np.stack([central(f, args, 4, k) for k in range(3)], 1)),
        "Jd": (J["Jd"], central(f, args, 2, None)),
        "Jn": (J["Jn"], np.stack([central(f, args, 3, k) for k in range(3)], 1)),
    }
    if lever:
        blocks["Jt"] = (J["Jt"], np.stack([central(f, args, 5, k) for k in range(3)], 1))
    for name, (ana, num) in blocks.items():
        scale = np.abs(num).max()
        dev = np.abs(ana - num).max() / scale
        print(f"{scene} {solver} {name}: max |analytic - central| / max = {dev:.3e}")
        assert dev < 1e-6, (name, dev)
    # exactly linear inputs: a finite step
    rng = np.random.default_rng(5)
    du = rng.normal(0, 0.05, u.shape); dw = rng.normal(0, 0.2, 3); dd = 0.37
    v0 = f(*args)
    for name, got, pred in (("u", f(x, u + du, d, n, om, t) - v0, np.einsum("jnc,nc->j", J["Ju"], du)),
                            ("omega", f(x, u, d, n, om + dw, t) - v0, J["Jw"] @ dw),
                            ("d", f(x, u, d + dd, n, om, t) - v0, J["Jd"] * dd)):
        dev = np.abs(got - pred).max() / max(np.abs(got).max(), 1e-300)
        print(f"{scene} {solver} finite step in {name}: {dev:.3e}")
        assert dev < 1e-10, (name, dev)


@pytest.mark.parametrize("variant", [cr.NODE, cr.SIM])
def test_residual_mode_is_the_textbook_covariance(sweeps, variant):
    x, u, d, n, om, t = scene12()
    X, b, ndotp = eo._system(x, u, n, om)
    if variant == cr.SIM:
        A = (X * ndotp[:, None, None]).reshape(-1, 3); B = b.reshape(-1) * d
    else:
        A = X.reshape(-1, 3); B = (b / ndotp[:, None]).reshape(-1) * d
    v, R, rank, s = np.linalg.lstsq(A, B, rcond=None)
    s2 = float(R[0]) / (2 * len(x) - 3)
    ref = s2 * np.linalg.inv(A.T @ A)
    rec = cr.covariance(variant, x, u, d, n, om, cr.sigmas(), cr.RESIDUAL)
    assert rec[13] == 0 and abs(rec[12] - s2) <= 1e-12 * s2
    assert np.abs(cr.untri(rec[0:6]) - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.array_equal(rec[0:6], rec[6:12]) and rec[17] == 0 and abs(rec[16] - np.trace(ref)) <= 1e-12 * np.trace(ref)
    # the common-mode terms stay as given
    sg = cr.sigmas(sigma_d=0.05, sigma_omega=(0.01, 0.02, 0.03))
    both = cr.covariance(variant, x, u, d, n, om, sg, cr.RESIDUAL)
    prop = cr.covariance(variant, x, u, d, n, om, sg, cr.PROPAGATE)
    np.testing.assert_allclose(both[0:6] - rec[0:6], prop[0:6], rtol=1e-9, atol=1e-18)
    # two points: 2m - 3 = 1 is enough; one point is void
    assert cr.covariance(variant, x[:1], u[:1], d, n, om, cr.sigmas(), cr.RESIDUAL, rank=2)[13] == 1


SWEEPS = {   # axis file -> the sigma a step sets (simulation.sweep_step)
    "effect_of_flow_errors": lambda i: dict(flow_sig=0.001 * i, position_sig=np.sqrt(2) / 1000 * i),
    "effect_of_distance_error": lambda i: dict(height_sig=0.001 * i),
    "effect_o_ang_vel_error": lambda i: dict(ang_vel_sig=0.001 * i),
    "effect_of_translation_error": lambda i: dict(translation_sig=0.001 * i),
}
DEFAULT_SIGMAS = dict(ang_vel_sig=0.00071, translation_sig=0.005, height_sig=0.01, flow_sig=0.056 * np.sqrt(2) * 1.23,
                      position_sig=0.056 * 1.23, normal_sig=0.00065)      # simulation.py:166-171


def predicted_std(x, u, step_sigmas):
    sg = dict(DEFAULT_SIGMAS); sg.update(step_sigmas)
    T = TRUTH
    # of_simulation discards its normal draw (simulation.py:45-46): sigma_normal = 0
    s = cr.sigmas(sigma_flow=sg["flow_sig"], sigma_pos=sg["position_sig"], sigma_d=sg["height_sig"], sigma_omega=sg["ang_vel_sig"],
                  sigma_offset=sg["translation_sig"])
    return cr.predict_std(cr.SIM, x, u, T["d"], T["n"], T["omega"], s, t=T["t"])


@pytest.mark.parametrize("name", sorted(SWEEPS))
def test_recorded_monte_carlo_sweeps_are_predicted(sweeps, name):
    x = centred(sweeps["points_raw"])
    T = TRUTH
    u = eo.generate_test_data(x, T["v"], T["omega"], T["d"], T["n"], T["t"])
    saved = sweeps[name]
    std_rec = saved[300:].reshape(100, 3)
    steps = np.arange(1, 100)
    pred = np.array([predicted_std(x, u, SWEEPS[name](i)) for i in steps])
    ratio = std_rec[steps] / pred
    rms = np.sqrt((std_rec[steps] ** 2).mean(0) / (pred ** 2).mean(0))
    outside = int(np.sum(np.abs(ratio - 1.0) > 0.35))
    print(f"{name}: mean ratio {ratio.mean():.3f}, rms ratio per component {np.round(rms, 3)}, outside +-35 %: {outside} of {ratio.size}")
    assert np.all((rms >= 0.80) & (rms <= 1.25)), rms
    assert outside <= 0.02 * ratio.size, outside


def test_structure(sweeps):
    x, u, d, n, om, t = scene12()
    R = eo.quat_to_rot(0.1, -0.05, 0.2, np.sqrt(1 - 0.01 - 0.0025 - 0.04))
    base = dict(sigma_flow=0.002, sigma_pos=0.003, sigma_d=0.04, sigma_omega=(0.01, 0.02, 0.015), sigma_normal=0.004, sigma_offset=0.006)
    for variant in (cr.NODE, cr.SIM):
        rec = cr.covariance(variant, x, u, d, n, om, cr.sigmas(**base), t=t, R=R)
        assert rec[13] == 0
        for sl in (slice(0, 6), slice(6, 12)):
            C = cr.untri(rec[sl])
            assert np.array_equal(C, C.T) and np.linalg.eigvalsh(C).min() >= -1e-15 * np.abs(C).max()
        assert abs(rec[16:21].sum() - np.trace(cr.untri(rec[0:6]))) <= 1e-12 * rec[16:21].sum()
        for j, key in enumerate(cr.SHARE_KEYS):
            dbl = dict(base); dbl[key] = tuple(2 * s for s in base[key]) if key == "sigma_omega" else 2 * base[key]
            r2 = cr.covariance(variant, x, u, d, n, om, cr.sigmas(**dbl), t=t, R=R)
            for k in range(6):
                want = 4.0 * rec[16 + k] if k == j else rec[16 + k]
                assert abs(r2[16 + k] - want) <= 1e-12 * abs(want), (key, k)
        # a rotation leaves the trace of C_uav alone; without a lever arm C_uav = C_v
        plain = cr.covariance(variant, x, u, d, n, om, cr.sigmas(**base))
        assert np.array_equal(plain[0:6], plain[6:12]) and plain[21] == 0
        norot = cr.covariance(variant, x, u, d, n, om, cr.sigmas(**base), t=t)
        assert abs(np.trace(cr.untri(norot[6:12])) - np.trace(cr.untri(rec[6:12]))) <= 1e-12 * np.trace(cr.untri(rec[6:12]))
    # void: rank below 3, no points, d = 0
    assert np.array_equal(cr.covariance(cr.NODE, x[:1], u[:1], d, n, om, cr.sigmas(**base), rank=2), cr.void_record())
    assert np.array_equal(cr.covariance(cr.NODE, x, u, d, n, om, cr.sigmas(**base), valid=np.zeros(12)), cr.void_record())
    assert np.array_equal(cr.covariance(cr.NODE, x, u, 0.0, n, om, cr.sigmas(**base)), cr.void_record())


def test_filter_r_with_a_void_covariance_is_the_constant_r_filter():
    rng = np.random.default_rng(3)
    H = np.vstack([np.eye(3, 6), np.eye(3, 6)]); Rm = 10.0 * np.eye(6)
    A = rng.normal(size=(6, 6)); P = A @ A.T + np.eye(6); x = rng.normal(size=6); z = rng.normal(size=6)
    xa, Pa, nis, gated = cr.kf_correct_cov(x, P, H, Rm, z, cov_rec=cr.void_record(), filter_r=True, r_floor=0.5)
    xb, Pb = eo.kf_correct(x, P, H, Rm, z)
    assert np.array_equal(xa, xb) and np.array_equal(Pa, Pb) and gated == 0 and nis > 0
    rec = np.zeros(24); rec[0:6] = cr.tri(0.01 * np.eye(3)); rec[6:12] = cr.tri(0.04 * np.eye(3))
    Re = cr.r_eff(Rm, rec, -1.0, 1, 0.5)
    assert np.allclose(Re[:3, :3], 0.54 * np.eye(3)) and np.array_equal(Re[3:, 3:], Rm[3:, 3:]) and not Re[:3, 3:].any()
    xg, Pg, nis_g, gated = cr.kf_correct_cov(x, P, H, Rm, z, cov_rec=rec, filter_r=True, nis_max=1e-300)
    assert gated == 1 and np.array_equal(xg, x) and np.array_equal(Pg, P)
    xh, Ph, nis_h, gated = cr.kf_correct_cov(x, P, H, Rm, z, cov_rec=rec, filter_r=True, nis_max=1e300)
    x0, P0, nis_0, _ = cr.kf_correct_cov(x, P, H, Rm, z, cov_rec=rec, filter_r=True)
    assert gated == 0 and np.array_equal(xh, x0) and np.array_equal(Ph, P0) and nis_h == nis_0


def test_stream_loop_at_an_unsolved_step():
    """CovStreamLoop.step with a record whose slot 15 is 0 (the step did not solve: v = 0, rank 0): the cov record is void with NIS
    and gate 0, the filter stays at its prediction, fused[7] is 0 - and the next, solved, step corrects from that prediction."""
    from types import SimpleNamespace
    import joint_reference as jr
    from test_joint_reference import pixel_points, sensor_row
    x, u, d, nrm, om0, v, om = jr.scene(65, 1065)
    sr = sensor_row(d, nrm, om)
    prev, nxt = pixel_points(x, u, sr)
    keep = np.ones(65, np.uint8); keep[7::9] = 0
    model = SimpleNamespace(x0=np.zeros(3), P0=1e-4 * np.eye(3), F=np.eye(3), Q=1e-6 * np.eye(3), B=np.eye(3), nc=3, H=np.eye(3), R=1e-4 * np.eye(3),
                            nm=3, ns=3)
    cfg = dict(mode=cr.PROPAGATE, sigma_flow=0.3, sigma_pos=0.5, sigma_d=0.04, sigma_omega=(0.01, 0.02, 0.015), sigma_normal=0.004, sigma_offset=0.006,
               filter_r=True, r_floor=1e-8)
    loop = cr.CovStreamLoop(model, cfg, -1.0, 1)
    control = np.array([1e-3, -2e-3, 5e-4])
    unsolved = np.zeros(16); unsolved[11] = np.count_nonzero(keep)
    srn = sr.copy(); srn[0] = np.nan                             # the dropout that left the step unsolved
    cv, xk, Pk, fused = loop.step(prev, nxt, keep, srn, unsolved, control)
    xp, Pp = eo.kf_predict(np.zeros(3), 1e-4 * np.eye(3), model.F, model.Q, model.B, control)
    assert np.array_equal(cv, cr.void_record()) and cv[14] == 0 and cv[15] == 0
    assert np.array_equal(xk, xp) and np.array_equal(Pk, Pp)
    assert np.array_equal(fused, np.concatenate([xp, np.zeros(3), [np.trace(Pp), 0.0]]))
    vs, rss, rank = jr.plain_solve(jr.NODE, *[a[keep.astype(bool)] for a in ((nxt - [640.0, 480.0]) * 1e-3, (nxt.astype(np.float64) - prev) * 1e-3)],
                                   d, nrm, om)
    rec = np.zeros(16); rec[0:3] = vs; rec[3] = rss; rec[4] = rank; rec[8:11] = vs; rec[15] = 1.0
    cv, xk, Pk, fused = loop.step(prev, nxt, keep, sr, rec, control)
    xp2, Pp2 = eo.kf_predict(xp, Pp, model.F, model.Q, model.B, control)
    assert cv[13] == 0 and cv[14] > 0 and fused[7] == 1 and not np.array_equal(xk, xp2)
    xr, Pr, nis, gated = cr.kf_correct_cov(xp2, Pp2, model.H, model.R, -vs, cov_rec=cv, z_sign=-1.0, z_source=1, filter_r=True, r_floor=1e-8)
    assert np.array_equal(xk, xr) and np.array_equal(Pk, Pr) and nis == cv[14]
