"""The robust velocity solve of include/ofk.h (ofk_set_robust) restated in numpy through oracle.estimation_oracle: the sampled
least-median-of-squares start, the reweighting rounds, the outputs.  Normal-equation route with the rank rule of DESIGN.md section 2
(an eigenvalue counts when it exceeds eps * rows * lambda_max).  Test infrastructure only; the product never imports it.

The moving-object experiment (scenes(), experiment()) lives here too, because the CPU and the GPU tests run the same scenes.
Measured with the committed code on the CPU oracle chain (tests/test_robust_reference.py prints them), 8 seeds per size:
    object 160x220 (10-13 % of the tracked corners): plain 0.3975-0.6188   robust 0.0045-0.0050
    object 260x330 (26-32 %):                        plain 0.9487-1.2293   robust 0.0045-0.0050
    object 300x400 (38-43 %):                        plain 1.4161-1.5864   robust 0.0046-0.0078
    no object:                                       plain 0.0057-0.0332   robust 0.0046-0.0049
every object corner ends at weight 0 except 4 and 1 corners in two of the 300x400 scenes
(relative error |v_obs - v| / |v| against the renderer's truth; TUKEY, c 4.685, 64 hypotheses, 5 rounds)."""
import numpy as np

from oracle import estimation_oracle as eo

OFF, HUBER, TUKEY = 0, 1, 2
NODE, SIM, OFMODULE = 0, 1, 2
MIN_POINTS = 8
EPS = 2.220446049250313e-16

# the experiment's conditions (the issue's): plain error at least PLAIN_MIN and robust error at most ROBUST_MAX with an object in view,
# robust <= plain + NO_OBJECT_SLACK without one
PLAIN_MIN, ROBUST_MAX, NO_OBJECT_SLACK = 0.2, 0.03, 1e-3
OBJECT_SIZES = ((160, 220), (260, 330), (300, 400))
SCENE_SEEDS = tuple(range(20, 28))
EXPERIMENT = dict(loss=TUKEY, c=4.685, iters=5, hypotheses=64, seed=0x1234ABCD5678)


def system(variant, x, u, d, n, omega, wgt=None):
    """A [m,3,3], B [m,3] of the kept points: A_i = sA [p]x, B_i = sB [p]x q (ofk.h's three systems)."""
    x = np.asarray(x, np.float64).reshape(-1, 2); u = np.asarray(u, np.float64).reshape(-1, 2)
    if variant == OFMODULE:
        X, b, ndp = eo._system(x, u, n, np.zeros(3))
        sA = 1.0 / np.asarray(wgt, np.float64); sB = sA / ndp
    else:
        X, b, ndp = eo._system(x, u, n, omega)
        if variant == SIM:
            sA = ndp; sB = np.full(len(x), float(d))
        else:
            sA = np.ones(len(x)); sB = float(d) / ndp
    return X * sA[:, None, None], b * sB[:, None]


def weighted_solve(A, B, w):
    """v, rank, singular values of the weighted normal equations; rows = 3 * (points with w > 0)."""
    M = np.einsum("n,nij,nik->jk", w, A, A)
    g = np.einsum("n,nij,ni->j", w, A, B)
    lam, Q = np.linalg.eigh(M)
    lam = lam[::-1]; Q = Q[:, ::-1]
    rows = 3.0 * float(np.count_nonzero(w > 0))
    tol = lam[0] * EPS * max(rows, 3.0)
    v = np.zeros(3); rank = 0
    for k in range(3):
        if lam[k] > tol and lam[k] > 0:
            v += Q[:, k] * (Q[:, k] @ g) / lam[k]
            rank += 1
    return v, rank, np.sqrt(np.maximum(lam, 0.0))


def rho2(A, B, v):
    r = A @ v - B
    return np.einsum("ni,ni->n", r, r)


def sel(a):
    """The element of index len(a) // 2 of a sorted ascending (an element of the set)."""
    return np.sort(a)[len(a) // 2]


def sample(seed, problem, hypotheses, m):
    """(i, j) of the hypotheses 0..K-1: Philox4x32-10(counter (h, problem, 0, 0), key (seed low, seed high))."""
    h = np.arange(int(hypotheses), dtype=np.uint64)
    x0, x1, _, _ = eo.philox4x32_10(h, np.full_like(h, int(problem)), np.zeros_like(h), np.zeros_like(h), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    i = (x0 % np.uint64(m)).astype(np.int64)
    j = (x1 % np.uint64(m - 1)).astype(np.int64)
    j += j >= i
    return i, j


def weights_of(loss, r2, c, s):
    t = np.sqrt(r2) / (c * s)
    if loss == HUBER:
        return np.where(t <= 1.0, 1.0, 1.0 / np.maximum(t, 1e-300)), t
    return np.where(t < 1.0, (1.0 - t * t) ** 2, 0.0), t


def robust_solve(variant, x, u, d, n, omega, wgt=None, valid=None, loss=TUKEY, c=4.685, iters=5, hypotheses=64, seed=0, problem=0,
                 min_cnt=0, force_hyp=None):
    """The estimator on one problem.  valid: which of the points are kept.  force_hyp: start from this hypothesis instead of the best
    one (the comparison's allowance for a device that broke a near-tie the other way).
    Returns v, r, rank, s[3], cnt, weights [n] (0 for points not kept), stats [8], and for the comparison's conditions the scores of
    all hypotheses (inf for void ones), gap = relative distance of the two best scores, tmin = the smallest |t_i - 1| met."""
    x = np.asarray(x, np.float64).reshape(-1, 2); u = np.asarray(u, np.float64).reshape(-1, 2)
    npts = len(x)
    keep = np.ones(npts, bool) if valid is None else np.asarray(valid).astype(bool).ravel()
    idx = np.flatnonzero(keep)
    m = len(idx)
    weights = np.zeros(npts)
    out = dict(scores=np.zeros(0), gap=np.inf, tmin=np.inf, near=0)
    if m == 0 or not m > min_cnt:
        out.update(v=np.zeros(3), r=0.0, rank=0, s=np.zeros(3), cnt=float(m), weights=weights + keep,
                   stats=np.array([0.0, m, m, m, -1, 0.0, 0, 1], np.float64))
        return out
    A, B = system(variant, x[idx], u[idx], d, n, omega, None if wgt is None else np.asarray(wgt, np.float64).ravel()[idx])
    w = np.ones(m)
    v, rank, sv = weighted_solve(A, B, w)
    s = 0.0; hyp = -1; score = 0.0; done = 0; flag = 0
    if m < MIN_POINTS:
        flag = 1
    else:
        if hypotheses > 0:
            hi, hj = sample(seed, problem, hypotheses, m)
            scores = np.full(hypotheses, np.inf); vs = np.zeros((hypotheses, 3))
            for h in range(hypotheses):
                wh = np.zeros(m); wh[hi[h]] = 1.0; wh[hj[h]] = 1.0
                vh, rk, _ = weighted_solve(A, B, wh)
                if rk == 3:
                    vs[h] = vh; scores[h] = sel(rho2(A, B, vh))
            out["scores"] = scores
            fin = np.unique(scores[np.isfinite(scores)])        # a pair drawn twice scores the same bits twice: no near-tie, "ties to the smaller h"
            if len(fin) >= 2:
                out["gap"] = (fin[1] - fin[0]) / fin[1] if fin[1] > 0 else 0.0
            if np.isfinite(scores).any():
                hyp = int(np.argmin(scores)) if force_hyp is None else int(force_hyp)   # argmin: the first of equal minima
                score = float(scores[hyp]); v = vs[hyp].copy()
        bb = float(np.einsum("ni,ni->", B, B))
        for _ in range(iters):
            r2 = rho2(A, B, v)
            s = 1.4826 * np.sqrt(sel(r2))
            if not s * s > 1e-24 * bb / m:
                flag = 2
                break
            wn, t = weights_of(loss, r2, c, s)
            out["tmin"] = min(out["tmin"], float(np.min(np.abs(t - 1.0))))
            out["near"] = max(out["near"], int(np.count_nonzero(np.abs(t - 1.0) < 1e-9)))
            v2, rk, sv2 = weighted_solve(A, B, wn)
            if rk < 3:
                flag = 3
                break
            v, rank, sv, w = v2, rk, sv2, wn
            done += 1
    weights[idx] = w
    cnt = float(np.count_nonzero(w > 0))
    out.update(v=v, r=float(w @ rho2(A, B, v)), rank=rank, s=sv, cnt=cnt, weights=weights,
               stats=np.array([s, w.sum(), cnt, m, hyp, score, done, flag], np.float64))
    return out


# ------------------------------------------------------------------------------------------------ the moving-object experiment
TRUTH = dict(v=(0.004, -0.003, 0.002), omega=(0.003, -0.002, 0.004), d=1.0)


def scene(synth, seed, size):
    """synth.render_pair 480x640 with (size = (oh, ow)) a textured rectangle pasted at (60, 80) in prev and (65, 73) in next: an object
    that moves by (-7, +5) px on its own.  size None: the plain pair."""
    pair = synth.render_pair(480, 640, seed, margin=96, **TRUTH)
    prev, nxt = pair["prev"].copy(), pair["next"].copy()
    if size is not None:
        oh, ow = size
        tex = synth.render_pair(oh + 40, ow + 40, seed + 100, margin=96)["prev"]
        prev[60:60 + oh, 80:80 + ow] = tex[20:20 + oh, 20:20 + ow]
        nxt[65:65 + oh, 73:73 + ow] = tex[20:20 + oh, 20:20 + ow]
    return pair, prev, nxt


def on_object(pts, size, row=60, col=80):
    if size is None:
        return np.zeros(len(pts), bool)
    p = np.asarray(pts, np.float64).reshape(-1, 2)
    return (p[:, 0] >= col) & (p[:, 0] < col + size[1]) & (p[:, 1] >= row) & (p[:, 1] < row + size[0])


def rel_err(v, truth):
    truth = np.asarray(truth, np.float64)
    return float(np.linalg.norm(np.asarray(v) - truth) / np.linalg.norm(truth))


def check_experiment(size, plain, robust, tag=""):
    """The experiment's two conditions for one scene."""
    if size is not None:
        assert plain >= PLAIN_MIN, (tag, "plain error", plain)
        assert robust <= ROBUST_MAX, (tag, "robust error", robust)
    else:
        assert robust <= plain + NO_OBJECT_SLACK, (tag, plain, robust)
