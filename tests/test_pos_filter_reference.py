"""The numpy restatement of the position filter (tests/pos_filter_reference.py, include/ofk.h: ofk_set_pos_filter) against an
independent dense textbook form, its invariants, and the experiment behind the README's figures (CPU-only).

Measured with this restatement (units of the height d; 12 000 steps, a re-key every 10 steps, sigma_D 1e-3 of whose variance half is
the key pixels' share, sigma_v 1e-3, a velocity that walks by 2e-3 per step, a fix of sigma 0.05 every 30 steps; seeds 0-7 pooled;
the filter with sigma_v 1e-3, q_v 2e-3 and the defaults otherwise):
  rms position error: filter 0.01490, the keyframe's own position 0.04669 (gain 3.13), the fixes alone 0.08726 (gain 5.86);
  without fixes: filter 0.03953 against the keyframe's 0.04669 (gain 1.18);
  pooled mean NEES of the position over the second half (3 is honest): 3.001 with share 0.5, 3.476 with share 0.
Asserted: each gain at half of what was measured, and the NEES at share 0.5 nearer to 3 than at share 0.
Wide priors: the pivots' floor of rule 6 is what carries the filter through priors of 1e6 and more (without it the displacement update
takes the rounding of P_pp - P_pc - P_cp + P_cc, entries of 1e12, for information, and P_pp ends at -1e7); with it P over the whole
sweep ends on the same values to nine digits, and its smallest eigenvalue never falls below -3.5e-16 of the largest entry it held."""
import numpy as np
import pytest

import pos_filter_reference as R

# the restatement against the dense form (in extended precision) over 300 random steps at priors 1e-4 ... 1e2: the largest deviation of x
# against |x|'s largest and of P against the largest entry of the P the step worked on is 3.89e-12 (prior 1, where P_vv falls from 1 to
# 4e-6 in one update); 16 x that.  Priors beyond 1e2 are left to the sweep below: there the dense form's outcomes differ from f64's.
TOL_DENSE = 16 * 3.89e-12


LD = np.longdouble                                               # the dense form's own rounding must not be what is measured


def inv3(S):
    """np.linalg.inv of a 3 x 3 in extended precision (numpy's own is f64 only): the adjugate over the determinant."""
    a, b, c, d, e, f, g, h, i = S.reshape(9)
    adj = np.array([[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f],
                    [d * h - e * g, b * g - a * h, a * e - b * d]], LD)
    return adj / (a * adj[0, 0] + b * adj[1, 0] + c * adj[2, 0])


def dense_step(x, P, fresh, s, v_uav, solved, key_rec, rw, inp):
    """Rules 2-7 as a textbook Kalman filter: full F, Q, H, the inverse of S, the Joseph form, in extended precision.  -> x, P, fresh,
    outcomes."""
    x, P, v_uav, key_rec, rw, inp = (np.asarray(a, LD) for a in (x, P, v_uav, key_rec, rw, inp))
    dt, I3, Z3 = LD(s["dt"]), np.eye(3, dtype=LD), np.zeros((3, 3), LD)
    F = np.block([[I3, dt * I3, Z3, Z3], [Z3, I3, -dt * I3, Z3], [Z3, Z3, I3, Z3], [Z3, Z3, Z3, I3]])
    Q = np.diag(np.array([s["q_p"]] * 3 + [s["q_v"]] * 3 + [s["q_b"]] * 3 + [0.0] * 3, LD) ** 2)
    u = np.zeros(12, LD)
    u[3:6] = np.where(np.isfinite(inp[0:3]), inp[0:3], 0.0)
    x = F @ x + u
    P = F @ P @ F.T + Q
    out = []

    def upd(x, P, H, z, Rm):
        S = H @ P @ H.T + Rm
        try:
            np.linalg.cholesky(S.astype(np.float64))
        except np.linalg.LinAlgError:
            return x, P, R.REFUSED
        y = z - H @ x
        Si = inv3(S)
        if s["nis_max"] > 0 and y @ Si @ y > s["nis_max"]:
            return x, P, R.GATED
        K = P @ H.T @ Si
        A = np.eye(12, dtype=LD) - K @ H
        Pn = A @ P @ A.T + K @ Rm @ K.T
        return x + K @ y, (Pn + Pn.T) / 2, R.APPLIED
    Hv = np.hstack([Z3, I3, Z3, Z3]); Hd = np.hstack([I3, Z3, Z3, -I3]); Hf = np.hstack([I3, Z3, Z3, Z3])
    o = R.NOT
    if s["sigma_v"] > 0 and solved and np.isfinite(v_uav).all():
        x, P, o = upd(x, P, Hv, v_uav, LD(s["sigma_v"]) ** 2 * I3)
    out.append(o)
    o = R.NOT
    if key_rec[3] == 0 and np.isfinite(key_rec[10:13]).all() and np.isfinite(key_rec[20:26]).all() and np.isfinite(rw).all():
        t = key_rec[20:26]
        CT = np.array([[t[0], t[1], t[2]], [t[1], t[3], t[4]], [t[2], t[4], t[5]]])
        Cm = LD(s["infl"]) ** 2 * rw @ CT @ rw.T + LD(s["floor"]) ** 2 * I3
        if fresh:
            P = P.copy(); P[9:12, 9:12] += LD(s["share"]) * Cm
            fresh = 0
        x, P, o = upd(x, P, Hd, key_rec[10:13], (1 - LD(s["share"])) * Cm)
    out.append(o)
    o = R.NOT
    if inp[3] != 0 and np.isfinite(inp[4:10]).all() and (inp[7:10] > 0).all():
        x, P, o = upd(x, P, Hf, inp[4:7], np.diag(inp[7:10] ** 2))
    out.append(o)
    if key_rec[9] != 0:
        T = np.eye(12, dtype=LD); T[9:12, 9:12] = 0; T[9:12, 0:3] = I3     # c = p
        x = T @ x; P = T @ P @ T.T
        fresh = 1
    return x, P, fresh, out


def random_inputs(rng, k, scale=1.0):
    v = rng.normal(0, 0.01, 3) * scale
    A = rng.normal(0, 1, (3, 3))
    CT = (A @ A.T + 0.5 * np.eye(3)) * 1e-6
    q, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
    kr = R.key_record(rng.normal(0, 0.02, 3) * scale, CT, flag=0 if rng.random() < 0.8 else 1, reason=0 if rng.random() < 0.8 else 2)
    inp = np.zeros(12)
    inp[0:3] = rng.normal(0, 0.001, 3)
    if rng.random() < 0.3:
        inp[3] = 1; inp[4:7] = rng.normal(0, 0.05, 3); inp[7:10] = rng.uniform(0.02, 0.1, 3)
    return v, rng.random() < 0.9, kr, q, inp


@pytest.mark.parametrize("prior", [1e-4, 1e-2, 1.0, 1e2])
def test_restatement_equals_the_dense_textbook_form(prior):
    rng = np.random.default_rng(int(np.log10(prior)) + 10)
    s = R.setting(dt=0.7, sigma_v=2e-3, floor=1e-4, infl=1.5, share=0.4, q_p=1e-4, q_v=1e-3, q_b=1e-5, p0_p=prior, p0_v=prior, p0_b=prior * 1e-2)
    st = R.new_state((1.0, -2.0, 0.5))
    R.start(st, s)
    x, P, fresh = st["x"].copy(), st["P"].copy(), 1
    worst = 0.0
    for k in range(300):
        v, solved, kr, rw, inp = random_inputs(rng, k)
        before = np.abs(P).max()
        rec = R.step(st, s, v, solved, kr, rw, inp)
        x, P, fresh, out = dense_step(x, P, fresh, s, v, solved, kr, rw, inp)
        assert [int(rec[25]), int(rec[30]), int(rec[35])] == out and st["istate"][1] == fresh
        x, P = x.astype(np.float64), P.astype(np.float64)
        dx = np.abs(st["x"] - x).max() / max(np.abs(x).max(), 1e-300)
        dP = np.abs(st["P"] - P).max() / max(np.abs(P).max(), before)   # against the scale of the P this step worked on
        worst = max(worst, dx, dP)
        x, P = st["x"].copy(), st["P"].copy()                    # one step's deviation, not a drift of two recursions
    print("largest deviation from the dense form", worst)
    assert worst <= TOL_DENSE


def test_behind_a_clone_the_displacement_sees_exactly_nothing():
    s0 = R.setting(share=0.0, floor=0.0, p0_p=0.3, q_p=1e-3)
    st = R.new_state()
    rng = np.random.default_rng(1)
    for k in range(5):
        R.step(st, s0, rng.normal(0, 0.01, 3), True, R.key_record(rng.normal(0, 0.01, 3), flag=0, reason=0), np.eye(3))
    R.clone(st)
    P = st["P"]
    assert np.array_equal(R.s_matrix(P, 0, 9, np.zeros((3, 3))), np.zeros((3, 3)))      # H_D P H_D^T, exactly
    keep = {k: v.copy() for k, v in st.items()}
    zero_cov = R.key_record((0.01, 0.0, 0.0), np.zeros((3, 3)))
    out, nis, y = R.update(st, 0, 9, zero_cov[10:13], np.zeros((3, 3)), 0.0)             # share = floor = 0 and C = 0: S is 0
    assert out == R.REFUSED and nis == 0.0 and np.isfinite(y).all()
    assert all(np.array_equal(st[k], keep[k]) for k in keep) and np.isfinite(st["P"]).all()
    # with a share the fresh step moves that part of C into P_cc, and S is C again
    s5 = R.setting(share=0.5)
    C = R.d_cov(R.key_record(C_T=np.diag([1e-6, 2e-6, 3e-6])), np.eye(3), s5)
    st["P"][9:12, 9:12] += s5["share"] * C
    S = R.s_matrix(st["P"], 0, 9, (1 - s5["share"]) * C)
    assert np.abs(S - C).max() <= 1e-12 * np.abs(C).max() + 4 * np.finfo(float).eps * np.abs(st["P"][0:3, 0:3]).max()


def test_a_held_block_stays_exactly_zero():
    s = R.setting(p0_b=0.0, q_b=0.0, p0_p=0.1, q_p=1e-4, nis_max=0.0)
    st = R.new_state()
    rng = np.random.default_rng(2)
    for k in range(200):
        v, solved, kr, rw, inp = random_inputs(rng, k)
        R.step(st, s, v, solved, kr, rw, inp)
        assert not st["P"][6:9, :].any() and not st["P"][:, 6:9].any() and not st["x"][6:9].any(), k
    assert st["istate"][4] > 50 and st["istate"][7] > 50 and st["istate"][10] > 20


@pytest.mark.parametrize("prior", [1e-4, 1e-2, 1.0, 1e2, 1e4, 1e6, 1e8])
def test_P_stays_symmetric_and_positive_over_2000_steps(prior):
    s = R.setting(p0_p=prior, p0_v=prior, p0_b=prior, q_b=1e-6, q_p=1e-5)
    st = R.new_state()
    rng = np.random.default_rng(3)
    least, held = np.inf, 0.0
    for k in range(2000):
        v, solved, kr, rw, inp = random_inputs(rng, k)
        R.step(st, s, v, solved, kr, rw, inp)
        P = st["P"]
        held = max(held, np.abs(P).max())
        assert np.isfinite(P).all() and (np.diag(P) > 0).all(), k
        least = min(least, np.linalg.eigvalsh(P).min() / held)
    # symmetric bit for bit behind an update; the predict and the clone keep it to the last bits of the larger entry
    assert np.abs(P - P.T).max() <= 4 * np.finfo(float).eps * np.abs(P).max()
    # Between a re-key and the next displacement update the clone is a copy of p, so P is singular by construction there: its smallest
    # eigenvalue is 0 up to the rounding of the updates, a few ulp of the largest entry P has held (measured: 1.6 ulp), never below
    assert least >= -64 * np.finfo(float).eps, least
    # every prior ends on the same P (to the fifth digit: the bias is hardly observed, so its prior leaves a trace in P_vv)
    assert np.allclose(np.diag(P)[[0, 3, 9]], [4.13093411e-05, 6.138239e-07, 3.98246622e-05], rtol=1e-4, atol=0.0)


@pytest.fixture(scope="module")
def figures():
    f = R.experiment()
    print({k: round(v, 5) for k, v in f.items()})
    return f


def test_the_filter_beats_the_keyframe_and_the_fixes(figures):
    f = figures
    assert f["key"] / f["filter"] >= 3.13 / 2
    assert f["fix"] / f["filter"] >= 5.86 / 2
    assert f["key"] / f["nofix"] >= 1 + 0.18 / 2      # without fixes: the gain over 1 at half


def test_modelling_the_shared_noise_makes_the_covariance_honest(figures):
    f = figures
    assert abs(f["nees_filter"] - 3.0) < abs(f["nees_filter_share0"] - 3.0)
