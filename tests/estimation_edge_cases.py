"""Ill-conditioned and degenerate inputs of the velocity solve (csrc/k_estimate.hip: solve_from_acc), with an exact reference.
Test infrastructure only, no GPU; tests/test_estimation_edge_cases.py pins this file, tests/test_gpu_estimation_edges.py uses it.

The device solves the 3 x 3 normal equations and cuts the rank where a singular-value ratio falls below sqrt(eps * 3N) (DESIGN.md
section 2, "rank"); np.linalg.lstsq works on A itself.  The two agree while kappa^2 * eps is small, kappa = s0 / s2 of A.  What is
here measures them both against exact_solve: the same normal equations in rational arithmetic.

  * the ladder     clusters of half-width h around (0.3, -0.2), h from 0.5 down to 1e-5 (kappa ~ 1.4 / h), 3 to 1025 points, the three
                   systems of ofk.h; the bound on a rank-3 v is  C * kappa^2 * eps * |v_exact|.
  * the window     sets whose kappa sits a factor 4 and 8 on either side of the rank cut thr = 1 / sqrt(eps * max(3N, 3)).
  * degenerates    single points, coincident points (two independent equations whatever their number: rank 2, minimum-norm v) and
                   pairs of f32 pixel neighbours.

Measured constants (tests/test_estimation_edge_cases.py prints and pins them; they are measured on the numpy restatement of the
device's route, robust_reference.weighted_solve, never on the device):
    worst |v - v_exact| / (kappa^2 eps |v_exact|) over the 90 rungs of the ladder: 3.52 (NODE 3.52, SIM 2.73, OFMODULE 3.06; lstsq
        itself stays within 1.4e-10 relative on every rung)                                     -> C_MEASURED, C = 16 x = 56.3
    worst |v - v_truncated lstsq| / |v_truncated lstsq| over every rank-2 case: 1.52e-14 (300 coincident points; the window sets, the
        single points and the pairs stay below 2e-15)                                            -> RANK2_MEASURED, RANK2_TOL = 16 x = 2.4e-13
The factor 16: the device adds in another order and diagonalises by cyclic Jacobi rather than LAPACK.

The rationals: fractions.Fraction reads every f64 exactly, but takes a gcd in every operation - minutes over the ladder once a
thousand different n.p stand in the denominators - so the sums are carried as unreduced integer triples (_Q) and rounded once at the
end; tests/test_estimation_edge_cases.py holds them to plain Fraction arithmetic, to the bit."""
import functools
from fractions import Fraction

import numpy as np

import robust_reference as rr
from oracle import estimation_oracle as eo

EPS = rr.EPS
NODE, SIM, OFMODULE = rr.NODE, rr.SIM, rr.OFMODULE
VARIANTS = (NODE, SIM, OFMODULE)

# measured: NODE 3.52 (1025 points, h 1e-2), SIM 2.73 (1025, 1e-4), OFMODULE 3.06 (1025, 1e-1), the worst rung of each;
# rank 2: 1.52e-14 (300 identical points, consistent flows; every other set stays below 2e-15)
C_MEASURED = 3.52
C = 16.0 * C_MEASURED
RANK2_MEASURED = 1.52e-14
RANK2_TOL = 16.0 * RANK2_MEASURED

TRUTH = dict(v=np.array([0.4, -0.3, 0.2]), omega=np.array([0.02, -0.01, 0.03]), d=1.7,
             nrm=np.array([0.06, -0.04, 1.0]) / np.linalg.norm([0.06, -0.04, 1.0]))
CENTRE = np.array([0.3, -0.2])
RUNGS = (0.5, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5)
COUNTS = (3, 64, 65, 257, 1025)                                  # below, at and across a wave, a 256-thread pass, four passes
FLOW_NOISE = 1e-5
WINDOW_COUNTS = (2, 3, 64)
WINDOW_FACTORS = (0.125, 0.25, 4.0, 8.0)                         # kappa / thr


# ------------------------------------------------------------------------------------------------ the exact reference
class _Q:
    """An exact rational n / (d 2^e) of Python integers, never reduced: fractions.Fraction takes a gcd in every operation, which
    costs minutes over the ladder once a thousand different n.p stand in the denominators.  Powers of two live in e, so sums of
    f64 values keep d = 1; only a division (by n.p, by a weight) makes d grow, and then it has to."""
    __slots__ = ("n", "d", "e")

    def __init__(self, n, d=1, e=0):
        self.n, self.d, self.e = n, d, e

    @staticmethod
    def of(a):
        n, d = Fraction(float(a)).as_integer_ratio()             # d is a power of two
        return _Q(n, 1, d.bit_length() - 1)

    def _sum(self, o, sign):
        e = max(self.e, o.e)
        a, b = self.n << (e - self.e), sign * o.n << (e - o.e)
        return _Q(a + b, self.d, e) if self.d == o.d else _Q(a * o.d + b * self.d, self.d * o.d, e)

    def __add__(self, o):
        return self._sum(o, 1)

    def __sub__(self, o):
        return self._sum(o, -1)

    def __mul__(self, o):
        return _Q(self.n * o.n, self.d * o.d, self.e + o.e)

    def __truediv__(self, o):
        sign = -1 if o.n < 0 else 1
        return _Q(sign * self.n * o.d, self.d * sign * o.n, self.e - o.e)

    def __float__(self):
        """Rounded once: the integers are shifted until the quotient has 64 bits, int / int rounds it correctly, ldexp is exact."""
        if self.n == 0:
            return 0.0
        n, d = self.n, self.d
        s = 64 - (abs(n).bit_length() - d.bit_length())
        if s > 0:
            n <<= s
        else:
            d <<= -s
        return float(np.ldexp(n / d, -self.e - s))


def _tree_sum(terms):
    """Pairwise: the operands of the late additions are the large ones, and there are few of those."""
    terms = list(terms)
    if not terms:
        return _Q(0)
    while len(terms) > 1:
        terms = [terms[k] + terms[k + 1] if k + 1 < len(terms) else terms[k] for k in range(0, len(terms), 2)]
    return terms[0]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _det3(m):
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def _exactly(values):
    """Every f64 of `values` (an array) as _Q."""
    return [_Q.of(a) for a in np.asarray(values, np.float64).ravel()]


class Exact:
    """v: the normal equations' solution rounded to f64 once (None where M is singular); bb = sum sB^2 |[p]x q|^2;
    rss(v): the exact residual sum of squares sum |sA [p]x v - sB [p]x q|^2 at a given f64 v, rounded once."""

    def __init__(self, rows, v, bb):
        self._rows, self.v, self.bb = rows, v, bb

    def rss(self, v):
        w = tuple(_exactly(v))
        terms = []
        for p, sA, sB, c in self._rows:
            pv = _cross(p, w)
            e = [sA * pv[k] - sB * c[k] for k in range(3)]
            terms.append(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
        return float(_tree_sum(terms))


def exact_solve(variant, x, u, d, n, omega, wgt=None, valid=None):
    """The normal equations of ofk.h's three systems (rows A_i = sA [p]x, B_i = sB [p]x q; NODE: q = u + [p]x omega, sA = 1,
    sB = d / (n.p); SIM: sA = n.p, sB = d; OFMODULE: q = u, sA = 1 / wgt_i, sB = sA / (n.p)) in exact rational arithmetic
    (_Q): every f64 input is taken exactly, M v = g is solved by Cramer's rule, the
    result is rounded to f64 once."""
    x = np.asarray(x, np.float64).reshape(-1, 2); u = np.asarray(u, np.float64).reshape(-1, 2)
    keep = np.flatnonzero(np.ones(len(x), bool) if valid is None else np.asarray(valid).astype(bool).ravel())
    m = len(keep)
    om = np.zeros(3) if variant == OFMODULE or omega is None else np.asarray(omega, np.float64)
    dd = 1.0 if variant == OFMODULE or d is None else float(d)
    ww = np.ones(m) if variant != OFMODULE else np.asarray(wgt, np.float64).ravel()[keep]
    flat = _exactly(np.concatenate([x[keep].ravel(), u[keep].ravel(), ww, np.asarray(n, np.float64), om, [dd]]))
    X, U, W = flat[:2 * m], flat[2 * m:4 * m], flat[4 * m:5 * m]
    nn, om, dd = flat[5 * m:5 * m + 3], flat[5 * m + 3:5 * m + 6], flat[5 * m + 6]
    one, zero = _Q(1), _Q(0)
    rows = []
    Mt = [[[] for _ in range(3)] for _ in range(3)]; gt = [[] for _ in range(3)]; bt = []
    for i in range(m):
        p = (X[2 * i], X[2 * i + 1], one)
        q3 = (U[2 * i], U[2 * i + 1], zero)
        ndp = nn[0] * p[0] + nn[1] * p[1] + nn[2]
        if variant == OFMODULE:
            q = q3; sA = one / W[i]; sB = sA / ndp
        else:
            w = _cross(p, om); q = (q3[0] + w[0], q3[1] + w[1], q3[2] + w[2])
            sA, sB = (ndp, dd) if variant == SIM else (one, dd / ndp)
        c = _cross(p, q)                                         # [p]x q
        pp = p[0] * p[0] + p[1] * p[1] + one
        sa2, sab = sA * sA, sA * sB
        for a in range(3):
            for b in range(a, 3):
                Mt[a][b].append(sa2 * ((pp if a == b else zero) - p[a] * p[b]))   # [p]x^T [p]x = |p|^2 I - p p^T
        t = _cross(c, p)                                         # [p]x^T c = -p x c
        for a in range(3):
            gt[a].append(sab * t[a])
        bt.append(sB * sB * (c[0] * c[0] + c[1] * c[1] + c[2] * c[2]))
        rows.append((p, sA, sB, c))
    M = [[None] * 3 for _ in range(3)]
    for a in range(3):
        for b in range(a, 3):
            M[a][b] = M[b][a] = _tree_sum(Mt[a][b])
    g = [_tree_sum(t) for t in gt]
    det = _det3(M) if m else _Q(0)
    v = None
    if det.n != 0:
        v = np.zeros(3)
        for k in range(3):
            Mk = [[g[r] if col == k else M[r][col] for col in range(3)] for r in range(3)]
            v[k] = float(_det3(Mk) / det)
    return Exact(rows, v, float(_tree_sum(bt)))


# ------------------------------------------------------------------------------------------------ numpy solvers
def rows_of(variant, x, u, d, n, omega, wgt=None):
    """A [3m, 3], B [3m] of robust_reference.system."""
    A, B = rr.system(variant, x, u, 1.0 if d is None else d, n, np.zeros(3) if omega is None else omega, wgt)
    return A.reshape(-1, 3), B.reshape(-1)


def lstsq_truncated(A, B, rank):
    """The SVD solution with the `rank` largest singular values kept; also the singular values."""
    U, s, Vt = np.linalg.svd(A, full_matrices=False)
    return Vt[:rank].T @ ((U[:, :rank].T @ B) / s[:rank]), s


def restatement(variant, x, u, d, n, omega, wgt=None, dtype=np.float64):
    """robust_reference.weighted_solve on the problem (the device's route in numpy): v, rank, s, rss.  dtype float32: a deliberately
    worse solver, M and g accumulated in float32 - the bounds must tell it from the real one."""
    A, B = rr.system(variant, x, u, 1.0 if d is None else d, n, np.zeros(3) if omega is None else omega, wgt)
    if dtype == np.float64:
        v, rank, s = rr.weighted_solve(A, B, np.ones(len(A)))
    else:
        A32, B32 = A.astype(np.float32), B.astype(np.float32)
        M = np.einsum("nij,nik->jk", A32, A32).astype(np.float64); g = np.einsum("nij,ni->j", A32, B32).astype(np.float64)
        lam, Q = np.linalg.eigh(M)
        lam = lam[::-1]; Q = Q[:, ::-1]
        tol = lam[0] * EPS * max(3.0 * len(A), 3.0)
        v = np.zeros(3); rank = 0
        for k in range(3):
            if lam[k] > tol and lam[k] > 0:
                v += Q[:, k] * (Q[:, k] @ g) / lam[k]; rank += 1
        s = np.sqrt(np.maximum(lam, 0.0))
    return v, rank, s, float(rr.rho2(A, B, v).sum())


# ------------------------------------------------------------------------------------------------ bounds
def v_bound(kappa, v_exact):
    return C * kappa * kappa * EPS * float(np.linalg.norm(v_exact))


def s_bound(kappa, s_ref):
    """Absolute bounds on s0, s1, s2: 1e-12 relative on the two large ones; lambda_3 carries an absolute error of order eps * lambda_0
    and the square root halves it: C kappa^2 eps relative on s2."""
    s_ref = np.asarray(s_ref, np.float64)
    return np.array([1e-12 * s_ref[0], 1e-12 * s_ref[1], C * kappa * kappa * EPS * s_ref[2]])


def rss_bound(r, bb):
    """The forward error of a sum of squares of differences whose terms cancel: r the exact value, bb = sum sB^2 |[p]x q|^2."""
    return 1e-8 * r + 64.0 * EPS * np.sqrt(r * bb) + 64.0 * EPS * EPS * bb


def thr(n):
    """kappa at the rank cut for n points."""
    return 1.0 / np.sqrt(EPS * max(3.0 * n, 3.0))


def expected_rank(kappa, n):
    """3 or 2 where kappa is a factor 4 clear of the cut, else None (only rank in {2, 3} is asserted there)."""
    return 3 if kappa <= thr(n) / 4.0 else 2 if kappa >= 4.0 * thr(n) else None


# ------------------------------------------------------------------------------------------------ the ladder
def _flows(variant, x, rng, noise=FLOW_NOISE):
    if variant == OFMODULE:                                      # no omega, no d in that system
        u = eo.generate_test_data(x, TRUTH["v"], np.zeros(3), 1.0, TRUTH["nrm"])
    else:
        u = eo.generate_test_data(x, TRUTH["v"], TRUTH["omega"], TRUTH["d"], TRUTH["nrm"])
    return u + rng.normal(0.0, noise, u.shape) if noise else u


def _problem(variant, x, u, wgt, t=None):
    """A problem with its references: kappa and s from lstsq's SVD of A, the exact solution."""
    d = None if variant == OFMODULE else TRUTH["d"]; om = None if variant == OFMODULE else TRUTH["omega"]
    A, B = rows_of(variant, x, u, d, TRUTH["nrm"], om, wgt)
    s = np.linalg.lstsq(A, B, rcond=None)[3]
    return dict(variant=variant, x=x, u=u, d=d, nrm=TRUTH["nrm"], omega=om, wgt=wgt, t=t, A=A, B=B, s=s, kappa=float(s[0] / s[2]),
                exact=exact_solve(variant, x, u, d, TRUTH["nrm"], om, wgt))


@functools.lru_cache(maxsize=None)
def ladder(variant, n):
    """The six rungs of (variant, n): fixed seed, computed once, shared - callers must not change them."""
    rng = np.random.default_rng(7000 + 100 * variant + n)
    out = []
    for k, h in enumerate(RUNGS):
        x = CENTRE + h * rng.uniform(-1.0, 1.0, (n, 2))
        wgt = rng.uniform(0.5, 2.0, n) if variant == OFMODULE else None
        t = rng.uniform(-0.1, 0.1, 3) if k % 2 else np.zeros(3)  # a lever arm on half of them
        p = _problem(variant, x, _flows(variant, x, rng), wgt, t)
        p["h"] = h
        out.append(p)
    return out


def solve_kwargs(variant, probs):
    """Context.velocity_solve's keyword arguments for a batch of problems of one variant and one point count."""
    kw = dict(nrm=np.stack([p["nrm"] for p in probs]))
    if variant == OFMODULE:
        kw["wgt"] = np.stack([p["wgt"] for p in probs])
    else:
        kw["d"] = np.array([p["d"] for p in probs]); kw["omega"] = np.stack([p["omega"] for p in probs])
        if all(p.get("t") is not None for p in probs):
            kw["t"] = np.stack([p["t"] for p in probs])
    return kw


def lever(p):
    """What the entry subtracts from v: omega x t."""
    return np.cross(p["omega"], p["t"]) if p["omega"] is not None and p.get("t") is not None else np.zeros(3)


# ------------------------------------------------------------------------------------------------ the rank window
def _kappa_of(x):
    A = eo._xhat(x).reshape(-1, 3)
    s = np.linalg.svd(A, compute_uv=False)
    return float(s[0] / s[2])


@functools.lru_cache(maxsize=None)
def window_case(n, factor):
    """n points around CENTRE whose kappa is factor * thr(n), found by bisection on the half-width h; the end of the last bracket that
    is on the far side of the cut is taken, so kappa / thr is at most `factor` below the cut and at least `factor` above it."""
    rng = np.random.default_rng(8000 + n)
    o = rng.uniform(-1.0, 1.0, (n, 2))
    target = factor * thr(n) * (1.001 if factor > 1.0 else 1.0 / 1.001)   # 0.1 % clear of the factor: another LAPACK moves kappa by 1e-9
    lo, hi = 1e-12, 1.0                                          # kappa(lo) > target > kappa(hi)
    assert _kappa_of(CENTRE + lo * o) > target > _kappa_of(CENTRE + hi * o)
    while hi / lo > 1.0 + 1e-4:
        mid = np.sqrt(lo * hi)
        if _kappa_of(CENTRE + mid * o) > target:
            lo = mid
        else:
            hi = mid
    x = CENTRE + (hi if factor < 1.0 else lo) * o
    p = _problem(NODE, x, _flows(NODE, x, np.random.default_rng(8100 + n + int(64 * factor))), None)
    p["factor"] = factor
    return p


# ------------------------------------------------------------------------------------------------ degenerate sets
F32_SCALING, F32_CX, F32_CY = 1.0 / 500.0, 320.0, 240.0


@functools.lru_cache(maxsize=None)
def degenerate_sets():
    """name -> dict(x [B, n, 2], flows = dict(consistent, random) of [B, n, 2]; pairs also pix [B, 2, 2] f32).  NODE system, the truth's
    sensors.  consistent: the truth's flow at each point (zero residual); random: N(0, 0.01) per component."""
    rng = np.random.default_rng(9000)
    sets = {"single": rng.uniform(-0.45, 0.45, (4096, 1, 2))}
    for k in (2, 5, 300):
        sets[f"identical_{k}"] = np.repeat(rng.uniform(-0.45, 0.45, (32, 1, 2)), k, axis=1)
    pix = np.zeros((64, 2, 2), np.float32)
    pix[:, 0, 0] = rng.uniform(280.0, 340.0, 64); pix[:, 0, 1] = rng.uniform(60.0, 420.0, 64)
    pix[:, 1] = pix[:, 0]
    up = np.nextafter(pix[:, 0], np.float32(np.inf))             # one f32 ulp on: in x for the even pairs, in y for the odd ones
    pix[0::2, 1, 0] = up[0::2, 0]; pix[1::2, 1, 1] = up[1::2, 1]
    sets["f32_pairs"] = (pix.astype(np.float64) - [F32_CX, F32_CY]) * F32_SCALING
    out = {}
    for name, x in sets.items():
        B, n, _ = x.shape
        cons = np.stack([eo.generate_test_data(x[b], TRUTH["v"], TRUTH["omega"], TRUTH["d"], TRUTH["nrm"]) for b in range(B)])
        out[name] = dict(x=x, flows=dict(consistent=cons, random=rng.normal(0.0, 0.01, (B, n, 2))))
    out["f32_pairs"]["pix"] = pix
    return out


def degenerate_reference(x, u):
    """One degenerate problem's reference: kappa, the rank the rule requires (None inside the window), and lstsq's solutions - the
    minimum-norm one at rank 2, the full one at rank 3."""
    A, B = rows_of(NODE, x, u, TRUTH["d"], TRUTH["nrm"], TRUTH["omega"])
    v2, s = lstsq_truncated(A, B, 2)
    kappa = float(s[0] / s[2]) if s[2] > 0 else np.inf
    return dict(A=A, B=B, s=s, kappa=kappa, rank=expected_rank(kappa, len(x)), v2=v2, v3=lstsq_truncated(A, B, 3)[0] if s[2] > 0 else None)


def check_solution(tag, out, ref, exact=None):
    """One device (or restatement) result out = (v[3], rss, rank, s[3]) against the rule: the rank the case requires, rank 2 against
    the truncated lstsq within RANK2_TOL, rank 3 against the exact solution (or full lstsq) within v_bound.  Returns the rank."""
    rank = int(out[4])
    want = ref["rank"]
    assert rank == want if want is not None else rank in (2, 3), (tag, "rank", rank, want, ref["kappa"])
    if rank == 2:
        err = np.linalg.norm(out[:3] - ref["v2"])
        assert err <= RANK2_TOL * np.linalg.norm(ref["v2"]), (tag, "rank 2", err, np.linalg.norm(ref["v2"]), ref["kappa"])
    else:
        v3 = exact.v if exact is not None and exact.v is not None else ref["v3"]
        err = np.linalg.norm(out[:3] - v3)
        assert err <= v_bound(ref["kappa"], v3), (tag, "rank 3", err, v_bound(ref["kappa"], v3), ref["kappa"])
    return rank


# ------------------------------------------------------------------------------------------------ the robust stage entry
ROBUST_N, ROBUST_M, ROBUST_PROBLEM = 80, 64, 0
ROBUST_SCALING, ROBUST_CX, ROBUST_CY = 1.0 / 500.0, 1024.0, 540.0
# seed 698: the smallest but one whose 64 hypotheses draw four of the 16 pairs and meet the comparison's conditions - two coincident
# pairs, a neighbour pair below the cut (lambda_3 / tol 0.036) and one above it (8.4)
ROBUST_SEED = 698
ROBUST_SETTING = dict(loss=rr.TUKEY, c=4.685, iters=5, hypotheses=64, seed=ROBUST_SEED)
ROBUST_INACCURATE = 1e-9                                         # a rank-3 hypothesis with C kappa^2 eps above the comparison's rtol


@functools.lru_cache(maxsize=None)
def robust_entry_case():
    """80 points of which a mask keeps 64: 8 coincident pairs, 4 pairs of f32 neighbours at 64-128 px (one ulp = 7.6e-6 px: below the
    rank cut), 4 at 1024-2048 px (1.2e-4 px: above it, kappa ~ thr / 3.5), 32 free points; a fifth of the flows moves otherwise, as in
    tests/test_gpu_robust.py.  Returns the problem (test_gpu_robust.make_problem's keys), valid, `special`: the kept-point
    numbers {i, j} of the 16 pairs, and the f32 pixels."""
    rng = np.random.default_rng(9500)
    pix = np.zeros((ROBUST_M, 2), np.float32)
    pix[:, 0] = rng.uniform(64.0, 1984.0, ROBUST_M); pix[:, 1] = rng.uniform(40.0, 1040.0, ROBUST_M)
    pix[16:24:2, 0] = rng.uniform(64.0, 127.0, 4); pix[24:32:2, 0] = rng.uniform(1024.0, 2047.0, 4)
    pix[1:32:2] = pix[0:32:2]
    pix[17:32:2, 0] = np.nextafter(pix[16:32:2, 0], np.float32(np.inf))
    order = rng.permutation(ROBUST_M)                            # kept number k holds pix[order[k]]
    where = np.argsort(order)
    special = frozenset(frozenset((int(where[2 * k]), int(where[2 * k + 1]))) for k in range(16))
    valid = np.zeros(ROBUST_N, np.uint8)
    valid[np.sort(rng.permutation(ROBUST_N)[:ROBUST_M])] = 1
    allpix = np.zeros((ROBUST_N, 2), np.float32)
    allpix[:, 0] = rng.uniform(64.0, 1984.0, ROBUST_N); allpix[:, 1] = rng.uniform(40.0, 1040.0, ROBUST_N)
    allpix[valid == 1] = pix[order]
    x = (allpix.astype(np.float64) - [ROBUST_CX, ROBUST_CY]) * ROBUST_SCALING
    u = eo.generate_test_data(x, TRUTH["v"] * 0.01, TRUTH["omega"] * 0.1, TRUTH["d"], TRUTH["nrm"])
    out = rng.permutation(ROBUST_N)[:ROBUST_N // 5]
    u[out] += np.array([-7.0, 5.0]) * ROBUST_SCALING
    u += rng.standard_normal((ROBUST_N, 2)) * 0.05 * ROBUST_SCALING
    p = dict(x=x, u=u, v=TRUTH["v"] * 0.01, om=TRUTH["omega"] * 0.1, d=TRUTH["d"], nrm=TRUTH["nrm"], wgt=np.ones(ROBUST_N), t=np.zeros(3))
    return p, valid, special, allpix


def robust_hypotheses(p, valid, seed):
    """Per sampled hypothesis of the reference: the pair (kept numbers), lambda_3 / tol, rank, C kappa^2 eps."""
    idx = np.flatnonzero(valid)
    A, B = rr.system(NODE, p["x"][idx], p["u"][idx], p["d"], p["nrm"], p["om"])
    hi, hj = rr.sample(seed, ROBUST_PROBLEM, ROBUST_SETTING["hypotheses"], len(idx))
    out = []
    for i, j in zip(hi, hj):
        w = np.zeros(len(idx)); w[i] = w[j] = 1.0
        _, rank, s = rr.weighted_solve(A, B, w)
        lam = s * s
        out.append(dict(pair=frozenset((int(i), int(j))), ratio=float(lam[2] / (lam[0] * EPS * 6.0)), rank=rank,
                        loss=float(C * EPS * lam[0] / lam[2]) if lam[2] > 0 else np.inf))
    return out
