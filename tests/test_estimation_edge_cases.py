"""CPU-only: pins tests/estimation_edge_cases.py - the exact reference against lstsq on the golden systems, the numpy restatement of the
device's route inside every bound, a float32 solver outside them, the window sets at the kappa they claim, the degenerate sets at rank
2 with lstsq's minimum-norm v, and the robust entry's case within the comparison's conditions.  Every listed case is used: nothing
here skips or filters."""
from fractions import Fraction

import numpy as np
import pytest

import estimation_edge_cases as ec
import robust_reference as rr


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge


def fraction_solve(variant, x, u, d, n, omega, wgt):
    """The same system written the long way in fractions.Fraction: the rows A_i = sA [p]x, B_i = sB [p]x q as matrices, M = sum A^T A,
    g = sum A^T B, Gaussian elimination; v and the residual sum of squares at v rounded to f64."""
    F = lambda a: Fraction(float(a))
    M = [[Fraction(0)] * 3 for _ in range(3)]; g = [Fraction(0)] * 3; rows = []
    for i in range(len(x)):
        px, py = F(x[i, 0]), F(x[i, 1])
        X = [[0, -1, py], [1, 0, -px], [-py, px, 0]]
        ndp = F(n[0]) * px + F(n[1]) * py + F(n[2])
        q = [F(u[i, 0]), F(u[i, 1]), Fraction(0)]
        if variant == ec.OFMODULE:
            sA = 1 / F(wgt[i]); sB = sA / ndp
        else:
            q = [q[r] + sum(X[r][c] * F(omega[c]) for c in range(3)) for r in range(3)]
            sA, sB = (ndp, F(d)) if variant == ec.SIM else (Fraction(1), F(d) / ndp)
        A = [[sA * X[r][c] for c in range(3)] for r in range(3)]
        B = [sB * sum(X[r][c] * q[c] for c in range(3)) for r in range(3)]
        rows.append((A, B))
        for a in range(3):
            g[a] += sum(A[r][a] * B[r] for r in range(3))
            for b in range(3):
                M[a][b] += sum(A[r][a] * A[r][b] for r in range(3))
    aug = [M[r] + [g[r]] for r in range(3)]
    for c in range(3):
        piv = next(r for r in range(c, 3) if aug[r][c] != 0)
        aug[c], aug[piv] = aug[piv], aug[c]
        for r in range(3):
            if r != c:
                f = aug[r][c] / aug[c][c]
                aug[r] = [a - f * b for a, b in zip(aug[r], aug[c])]
    v = np.array([float(aug[r][3] / aug[r][r]) for r in range(3)])
    vf = [F(c) for c in v]
    rss = sum((sum(A[r][c] * vf[c] for c in range(3)) - B[r]) ** 2 for A, B in rows for r in range(3))
    return v, float(rss), float(sum(B[r] ** 2 for _, B in rows for r in range(3)))


@pytest.mark.parametrize("variant", ec.VARIANTS)
def test_exact_solve_is_fraction_arithmetic(variant):
    """estimation_edge_cases carries its rationals unreduced for speed; the results are those of fractions.Fraction, to the bit."""
    rng = np.random.default_rng(50 + variant)
    for n, h in ((3, 0.5), (9, 1e-3), (17, 1e-5)):
        x = ec.CENTRE + h * rng.uniform(-1.0, 1.0, (n, 2)); u = ec._flows(variant, x, rng); wgt = rng.uniform(0.5, 2.0, n)
        ex = ec.exact_solve(variant, x, u, ec.TRUTH["d"], ec.TRUTH["nrm"], ec.TRUTH["omega"], wgt)
        v, rss, bb = fraction_solve(variant, x, u, ec.TRUTH["d"], ec.TRUTH["nrm"], ec.TRUTH["omega"], wgt)
        assert np.array_equal(ex.v, v) and ex.rss(v) == rss and ex.bb == bb, (variant, n, h, ex.v, v)


@pytest.mark.parametrize("N", [3, 4, 20, 200, 500, 2000])
def test_exact_solve_agrees_with_lstsq_on_the_golden_systems(golden, N):
    g = golden; p = f"g4_{N}_"
    x, u, n, om, d = g[p + "x"], g[p + "u"], g[p + "n"], g[p + "omega"], float(g[p + "d"])
    rng = np.random.default_rng(N)
    wgt = rng.uniform(0.5, 2.0, len(x))
    for variant in ec.VARIANTS:
        A, B = ec.rows_of(variant, x, u, d, n, om, wgt if variant == ec.OFMODULE else None)
        v, R, rank, s = np.linalg.lstsq(A, B, rcond=None)
        ex = ec.exact_solve(variant, x, u, d, n, om, wgt)
        assert rank == 3
        np.testing.assert_allclose(ex.v, v, rtol=1e-12, atol=1e-12 * np.linalg.norm(v))
        if N > 3:
            np.testing.assert_allclose(ex.rss(v), R[0], rtol=1e-9)
        np.testing.assert_allclose(ex.bb, B @ B, rtol=1e-12)
    valid = (rng.uniform(size=len(x)) < 0.6) | (np.arange(len(x)) < 3)
    a = ec.exact_solve(ec.NODE, x, u, d, n, om, valid=valid); b = ec.exact_solve(ec.NODE, x[valid], u[valid], d, n, om)
    assert np.array_equal(a.v, b.v) and a.bb == b.bb


def test_exact_solve_reports_a_singular_system():
    x = np.repeat([[0.25, -0.125]], 4, axis=0)
    assert ec.exact_solve(ec.NODE, x, np.full((4, 2), 0.5), 1.0, [0, 0, 1.0], np.zeros(3)).v is None


def ladder_rows(float32=False):
    for variant in ec.VARIANTS:
        for n in ec.COUNTS:
            for p in ec.ladder(variant, n):
                v, rank, s, rss = ec.restatement(variant, p["x"], p["u"], p["d"], p["nrm"], p["omega"], p["wgt"],
                                                 dtype=np.float32 if float32 else np.float64)
                yield p, n, v, rank, s, rss


def test_measured_constants():
    """The restatement inside every bound over the whole ladder, and the figures estimation_edge_cases.py quotes."""
    worst = {}
    for p, n, v, rank, s, rss in ladder_rows():
        ex = p["exact"]
        tag = (p["variant"], n, p["h"])
        ratio = np.linalg.norm(v - ex.v) / (p["kappa"] ** 2 * ec.EPS * np.linalg.norm(ex.v))
        worst[p["variant"]] = max(worst.get(p["variant"], 0.0), ratio)
        assert rank == 3, tag
        assert np.linalg.norm(v - ex.v) <= ec.v_bound(p["kappa"], ex.v), tag
        assert np.all(np.abs(s - p["s"]) <= ec.s_bound(p["kappa"], p["s"])), (tag, s, p["s"])
        r = ex.rss(v)
        assert abs(rss - r) <= ec.rss_bound(r, ex.bb), (tag, rss, r)
        assert np.linalg.norm(np.linalg.lstsq(p["A"], p["B"], rcond=None)[0] - ex.v) <= 1e-9 * np.linalg.norm(ex.v), tag   # lstsq: 1.4e-10 at worst
    print("worst err / (kappa^2 eps |v|) per variant", worst)
    # the figure is rounding error: another BLAS or SIMD width adds in another order and moves it, so it is held to a factor 2
    assert 0.5 * ec.C_MEASURED <= max(worst.values()) <= 2.0 * ec.C_MEASURED, "C_MEASURED is not what the ladder measures any more"
    assert ec.C == 16.0 * ec.C_MEASURED


def test_a_float32_solver_breaks_the_bound():
    broken = set()
    for p, n, v, rank, s, rss in ladder_rows(float32=True):
        if rank < 3 or np.linalg.norm(v - p["exact"].v) > ec.v_bound(p["kappa"], p["exact"].v):
            broken.add((p["variant"], n, p["h"]))
    for variant in ec.VARIANTS:
        for n in ec.COUNTS:
            for h in (1e-2, 1e-3, 1e-4):
                assert (variant, n, h) in broken, (variant, n, h)


@pytest.mark.parametrize("n", ec.WINDOW_COUNTS)
def test_window_sets_have_the_kappa_they_claim(n):
    worst2 = 0.0
    for f in ec.WINDOW_FACTORS:
        p = ec.window_case(n, f)
        r = p["kappa"] / ec.thr(n)
        assert (1.0 / r >= 4.0 and r >= 0.99 * f) if f < 1 else (r >= 4.0 and r <= 1.01 * f), (n, f, r)
        assert ec.expected_rank(p["kappa"], n) == (3 if f < 1 else 2)
        v, rank, s, rss = ec.restatement(ec.NODE, p["x"], p["u"], p["d"], p["nrm"], p["omega"])
        ref = dict(rank=ec.expected_rank(p["kappa"], n), kappa=p["kappa"], v2=ec.lstsq_truncated(p["A"], p["B"], 2)[0], v3=None)
        ec.check_solution((n, f), np.concatenate([v, [rss, rank], s]), ref, p["exact"])
        if rank == 2:
            worst2 = max(worst2, np.linalg.norm(v - ref["v2"]) / np.linalg.norm(ref["v2"]))
    print("rank 2 against truncated lstsq", worst2)
    assert worst2 <= 2.0 * ec.RANK2_MEASURED                    # rounding error: held to a factor 2 (see test_measured_constants)


@pytest.mark.parametrize("name", ("single", "identical_2", "identical_5", "identical_300", "f32_pairs"))
def test_degenerate_sets_on_the_restatement(name):
    st = ec.degenerate_sets()[name]
    worst2 = 0.0; seen = {}
    for flow, u in st["flows"].items():
        for b in range(len(st["x"])):
            ref = ec.degenerate_reference(st["x"][b], u[b])
            if name != "f32_pairs":
                assert ref["rank"] == 2, (name, b, ref["kappa"])     # coincident points: two independent equations
            v, rank, s, rss = ec.restatement(ec.NODE, st["x"][b], u[b], ec.TRUTH["d"], ec.TRUTH["nrm"], ec.TRUTH["omega"])
            rank = ec.check_solution((name, flow, b), np.concatenate([v, [rss, rank], s]), ref)
            seen[(ref["rank"], rank)] = seen.get((ref["rank"], rank), 0) + 1
            if rank == 2:
                worst2 = max(worst2, np.linalg.norm(v - ref["v2"]) / np.linalg.norm(ref["v2"]))
    print(name, "required / found ranks", seen, "rank 2 against truncated lstsq", worst2)
    assert worst2 <= 2.0 * ec.RANK2_MEASURED and ec.RANK2_TOL == 16.0 * ec.RANK2_MEASURED
    if name == "f32_pairs":                                     # one ulp at 300 px and scaling 1 / 500: right at the cut
        pix = st["pix"]
        step = pix[:, 1] - pix[:, 0]
        assert pix.dtype == np.float32 and np.all((step != 0).sum(axis=1) == 1) and np.array_equal(step[step != 0], np.spacing(pix[:, 0])[step != 0])
        assert np.all(step[0::2, 0] == np.spacing(np.float32(300.0)))
        assert np.array_equal(st["x"], (pix.astype(np.float64) - [ec.F32_CX, ec.F32_CY]) * ec.F32_SCALING)


def test_robust_entry_case_meets_the_comparison_conditions(built, ofk):
    p, valid, special, pix = ec.robust_entry_case()
    s = ec.ROBUST_SETTING
    assert int(valid.sum()) == ec.ROBUST_M and len(special) == 16
    i, j = ofk.robust_pairs(s["seed"], ec.ROBUST_PROBLEM, s["hypotheses"], ec.ROBUST_M)      # host only
    ri, rj = rr.sample(s["seed"], ec.ROBUST_PROBLEM, s["hypotheses"], ec.ROBUST_M)
    assert np.array_equal(i, ri) and np.array_equal(j, rj)
    drawn = [frozenset((int(a), int(b))) for a, b in zip(i, j)]
    assert sum(d in special for d in drawn) >= 4
    idx = np.flatnonzero(valid)
    for pr in special:                                           # the pairs are what they are said to be
        a, b = sorted(pr)
        dpx = np.abs(pix[idx[a]] - pix[idx[b]])
        assert dpx[1] == 0 and (dpx[0] == 0 or dpx[0] == np.spacing(min(pix[idx[a], 0], pix[idx[b], 0])))
    hyps = ec.robust_hypotheses(p, valid, s["seed"])
    ref = rr.robust_solve(rr.NODE, p["x"], p["u"], p["d"], p["nrm"], p["om"], valid=valid, loss=s["loss"], c=s["c"], iters=s["iters"],
                          hypotheses=s["hypotheses"], seed=s["seed"], problem=ec.ROBUST_PROBLEM)
    assert ref["gap"] >= 1e-6 and ref["near"] == 0 and ref["stats"][7] == 0
    best = ref["scores"][np.isfinite(ref["scores"])].min()
    kinds = set()
    for h, sc in zip(hyps, ref["scores"]):
        assert not 0.25 <= h["ratio"] <= 4.0, h                  # the device's rank cannot differ from the reference's
        assert (h["rank"] == 3) == bool(np.isfinite(sc))
        if h["rank"] == 3 and h["loss"] > ec.ROBUST_INACCURATE:  # its v may differ beyond the comparison's tolerance: it must not matter
            assert sc >= 10.0 * best, (h, sc, best)
            print("inaccurate hypothesis", sorted(h["pair"]), f"lambda_3/tol {h['ratio']:.2f} score / best {sc / best:.1f}")
        if h["pair"] in special:
            kinds.add("coincident" if h["ratio"] < 1e-3 else "below" if h["rank"] == 2 else "above")
    assert kinds == {"coincident", "below", "above"}, kinds
