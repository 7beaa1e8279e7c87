"""GPU parity of the small float64 kernels at the end of csrc/k_estimate.hip - k_feature_eval, k_d_split, k_kf, k_imu, k_imu_seq,
k_post_solve, k_flow_model, k_feasibility - at the inputs where their numpy originals behave specially (NaN, +-inf, ties, empty
sets), across the 64- and 256-thread block boundaries of their launches, and over the filter's dimension grid.  Every expected
value comes from oracle/estimation_oracle.py or from a closed form written here; every edge case is asserted ON THE ORACLE'S
OUTPUT before it is used, so a change to a generator cannot turn it into an ordinary case unnoticed.  Every linear system is well
conditioned by construction (cond(S) is asserted): what is tested is numpy's semantics, launch geometry and dimensions, at the
tolerances the project already uses for each kernel (tests/test_feature_eval.py, tests/test_gpu_estimation_parity.py)."""
import numpy as np
import pytest

from oracle import estimation_oracle as eo
from test_feature_eval import make_set
from test_gpu_estimation_parity import close

pytestmark = pytest.mark.gpu

IMG, FOCAL, DUMMY = (320, 240), 320.0, -1.0
W4 = [0.4, 0.3, 0.2, 0.1]
EPS = 2.220446049250313e-16


# ================================================================================================ feature_eval
def fe_set(rng, n, vel=(3.0, -2.0, 0.2), img=IMG):
    pos, old, pe, oe = make_set(rng, n, img)
    return dict(pos=pos, old=old, pe=pe, oe=oe, vel=np.array(vel, np.float64), vel_err=np.array([0.03, 0.02, 0.04]))


def fe_oracle(s, n=None, weight=W4, focal=FOCAL, img=IMG, dummy=DUMMY):
    n = len(s["pos"]) if n is None else n
    return eo.feature_eval(s["pos"][:n], s["pe"][:n], s["old"][:n], s["oe"][:n], s["vel"], s["vel_err"], focal, dummy, img, weight)


def fe_run(ctx, sets, counts=None, stride=None, weight=W4, focal=FOCAL, img=IMG, dummy=DUMMY):
    """The sets as one batch; slots past a set's data hold NaN, so a kernel that read them would show it."""
    B = len(sets)
    stride = max(max(len(s["pos"]) for s in sets), 1) if stride is None else stride
    pos = np.full((B, stride, 2), np.nan); old = np.full((B, stride, 2), np.nan); pe = np.full((B, stride), np.nan); oe = np.full((B, stride), np.nan)
    for b, s in enumerate(sets):
        m = len(s["pos"])
        pos[b, :m] = s["pos"]; old[b, :m] = s["old"]; pe[b, :m] = s["pe"]; oe[b, :m] = s["oe"]
    counts = np.array([len(s["pos"]) for s in sets], np.int32) if counts is None else np.asarray(counts, np.int32)
    vel = np.stack([s["vel"] for s in sets]); vel_err = np.stack([s["vel_err"] for s in sets])
    return ctx.feature_eval(pos, pe, old, oe, vel, vel_err, focal, dummy, img, weight, counts=counts)


def fe_check(out, b, c, ref):
    """Set b of a batch result against the oracle's tuple on its first c features, and the slots past them."""
    if c:
        h, he, imm, score, order = ref
        np.testing.assert_allclose(out["height"][b, :c], h, rtol=1e-14, atol=0, equal_nan=True)
        np.testing.assert_allclose(out["height_err"][b, :c], he, rtol=1e-13, atol=0, equal_nan=True)
        assert np.array_equal(out["immobile"][b, :c].astype(bool), imm)
        np.testing.assert_allclose(out["score"][b, :c], score, rtol=1e-12, atol=1e-15, equal_nan=True)
        assert np.array_equal(out["order"][b, :c], order), (b, c)
    assert np.all(out["order"][b, c:] == -1) and np.all(out["height"][b, c:] == 0) and np.all(out["height_err"][b, c:] == 0)
    assert np.all(out["score"][b, c:] == 0) and np.all(out["immobile"][b, c:] == 0)


def fe_check_all(ctx, sets, **kw):
    out = fe_run(ctx, sets, **kw)
    okw = {k: v for k, v in kw.items() if k in ("weight", "focal", "img", "dummy")}
    for b, s in enumerate(sets):
        fe_check(out, b, len(s["pos"]), fe_oracle(s, **okw))
    return out


@pytest.mark.parametrize("still", ["x", "y", "xy"])
def test_feature_eval_level_flight(gpu_ctx, still):
    """v_z == 0 and feature 4 without flow on one axis (or both): its height is inf and its variance holds e v_z / u = 0 / 0.  The
    oracle's np.amin / np.amax of the variances are NaN, so the height_err term is zero for all twelve features."""
    s = fe_set(np.random.default_rng(41), 12, vel=(2.0, 1.0, 0.0))
    if "x" in still:
        s["old"][4, 0] = s["pos"][4, 0]
    if "y" in still:
        s["old"][4, 1] = s["pos"][4, 1]
    h, he, imm, score, order = fe_oracle(s)
    assert np.isinf(h[4]) and np.isinf(h).sum() == 1 and np.isnan(he[4]) and np.isnan(he).sum() == 1
    assert np.isfinite(score).sum() == 11 and np.isnan(score[4]) and order[-1] == 4
    e = np.delete(he, 4)                                         # a range over the other eleven would not be zero: the term would show
    assert np.isfinite(e).all() and e.max() > e.min()
    fe_check_all(gpu_ctx, [s])
    other = fe_set(np.random.default_rng(42), 12)                # and beside an ordinary set: the NaN range belongs to one block
    fe_check_all(gpu_ctx, [other, s, other])


def test_feature_eval_nan_heights_scores_and_errors(gpu_ctx):
    rng = np.random.default_rng(43)
    # a stationary feature where f v_x - x v_z > 0 > f v_y - y v_z: height = 0.5 (inf - inf) = NaN, the height term is zero for the set
    a = fe_set(rng, 12, vel=(2.0, -1.0, 0.2))
    a["old"][4] = a["pos"][4]
    assert FOCAL * 2.0 - a["pos"][4, 0] * 0.2 > 0 > FOCAL * -1.0 - a["pos"][4, 1] * 0.2
    h, he, imm, score, order = fe_oracle(a)
    assert np.isnan(h).sum() == 1 and np.isnan(h[4]) and np.isinf(he).sum() == 1 and np.isfinite(score).sum() == 11 and order[-1] == 4
    # two and three NaN scores in one set: last, in index order
    b2 = fe_set(rng, 40, vel=(2.0, 1.0, 0.0)); b3 = fe_set(rng, 300, vel=(2.0, 1.0, 0.0))
    for k in (31, 7):
        b2["old"][k] = b2["pos"][k]
    for k in (299, 0, 256):
        b3["old"][k] = b3["pos"][k]
    o2, o3 = fe_oracle(b2), fe_oracle(b3)
    assert np.isnan(o2[3]).sum() == 2 and list(o2[4][-2:]) == [7, 31] and np.isnan(o3[3]).sum() == 3 and list(o3[4][-3:]) == [0, 256, 299]
    # NaN in pos_err of one feature: its variance is NaN and it is not immobile; the pos_err and height_err terms are zero for the
    # WHOLE set, that feature included (np.zeros_like), so every score stays finite
    c = fe_set(rng, 70)
    c["pe"][33] = np.nan
    oc = fe_oracle(c)
    assert np.isnan(oc[1]).sum() == 1 and np.isnan(oc[1][33]) and not oc[2][33] and np.isfinite(oc[0]).all() and np.isfinite(oc[3]).all()
    out = fe_check_all(gpu_ctx, [a, b2, b3, c])
    assert out["bad_height"]


def test_feature_eval_count_boundaries(gpu_ctx):
    """One batch, stride 1024, ragged counts around the 256-thread block: 1, 2, 255, 256, 257, 513, 1024, none, and a count above
    the stride (clamped to it)."""
    rng = np.random.default_rng(44)
    sizes = [1, 2, 255, 256, 257, 513, 1024, 0, 1024]
    sets = [fe_set(rng, n, vel=rng.normal(0, 1.0, 3) + [3.0, -2.0, 0.2]) for n in sizes]
    counts = np.array(sizes, np.int32); counts[-1] = 1024 + 77
    out = fe_run(gpu_ctx, sets, counts=counts, stride=1024)
    for b, s in enumerate(sets):
        fe_check(out, b, sizes[b], fe_oracle(s) if sizes[b] else None)
    # the empty set alone contributes nothing to bad_height; positive heights beside it keep the flag clear
    good = good_sets()
    assert not fe_run(gpu_ctx, [good[0], sets[7], good[1]], stride=8)["bad_height"]
    # stride 1: one feature, none, and a count above the stride
    one = [fe_set(rng, 1), fe_set(rng, 0), fe_set(rng, 1)]
    out = fe_run(gpu_ctx, one, counts=[1, 0, 5], stride=1)
    for b, s in enumerate(one):
        fe_check(out, b, len(s["pos"]), fe_oracle(s) if len(s["pos"]) else None)


def test_feature_eval_ties(gpu_ctx):
    rng = np.random.default_rng(45)
    f = fe_set(rng, 1)
    rep = {k: (np.repeat(v, 300, axis=0) if k in ("pos", "old", "pe", "oe") else v) for k, v in f.items()}
    o = fe_oracle(rep)
    assert np.all(o[3] == o[3][0]) and np.array_equal(o[4], np.arange(300))    # every range is zero: equal scores, identity order
    half = fe_set(rng, 150)
    dbl = {k: (np.concatenate([v, v]) if k in ("pos", "old", "pe", "oe") else v) for k, v in half.items()}
    o = fe_oracle(dbl)
    assert np.array_equal(o[3][:150], o[3][150:]) and np.all(o[4][1::2] - o[4][0::2] == 150)      # pairs (i, i + 150), the lower index first
    out = fe_check_all(gpu_ctx, [rep, dbl])
    assert np.array_equal(out["order"][0], np.arange(300))
    zero = fe_set(rng, 257)
    o = fe_oracle(zero, weight=[0, 0, 0, 0])
    assert np.all(o[3] == 0) and np.array_equal(o[4], np.arange(257))
    fe_check_all(gpu_ctx, [zero], weight=[0.0, 0.0, 0.0, 0.0])


def good_sets():
    """Three sets with positive heights only: flow and velocity of one sign, level flight."""
    rng = np.random.default_rng(46)
    sets = []
    for n in (3, 8, 5):
        s = fe_set(rng, n, vel=(2.0, 1.0, 0.0))
        s["old"] = s["pos"] - rng.uniform(1.0, 5.0, (n, 2))
        sets.append(s)
    return sets


def one_feature(pos, flow, vel):
    return dict(pos=np.array([pos], np.float64), old=np.array([pos], np.float64) - np.array([flow], np.float64), pe=np.array([0.1]),
                oe=np.array([0.1]), vel=np.array(vel, np.float64), vel_err=np.array([0.01, 0.01, 0.01]))


def test_feature_eval_bad_height_flag(gpu_ctx):
    """One flag per call, OR-ed over the sets: set by a NaN, a zero, a negative and a sub-epsilon height in ONE set among good ones
    (the reference raises ValueError there), clear for positive heights only."""
    good = good_sets()
    for s in good:
        assert np.all(fe_oracle(s, focal=100.0)[0] >= EPS)
    out = fe_check_all(gpu_ctx, good, focal=100.0)
    assert not out["bad_height"]
    bad = {
        "nan": one_feature((150.0, 110.0), (0.0, 0.0), (2.0, -1.0, 0.0)),       # inf - inf
        "zero": one_feature((200.0, 100.0), (3.0, 2.0), (2.0, 1.0, 1.0)),       # f v_x - x v_z = 100 * 2 - 200 = 0 on both axes
        "negative": one_feature((150.0, 110.0), (-3.0, -2.0), (2.0, 1.0, 0.0)),
        "tiny": one_feature((150.0, 110.0), (1.0, 1.0), (1e-19, 1e-19, 0.0)),   # 1e-17: positive and below the reference's epsilon
    }
    h = {k: fe_oracle(s, focal=100.0)[0][0] for k, s in bad.items()}
    assert np.isnan(h["nan"]) and h["zero"] == 0.0 and h["negative"] < 0 and 0 < h["tiny"] < EPS
    for k, s in bad.items():
        out = fe_check_all(gpu_ctx, [good[0], good[1], s, good[2]], focal=100.0)
        assert out["bad_height"], k


def test_feature_eval_dummy_coordinates_at_both_ends(gpu_ctx):
    """An immobile feature (found with the oracle) copied into the first and the last slot of a 257-feature set; with dummy_value
    equal to its old x, then its old y, both slots stop being immobile and nothing else changes."""
    rng = np.random.default_rng(47)
    s = fe_set(rng, 257)
    s["oe"][:] = 2.0                                             # loose observation error: some features pass the immobility test
    imm = fe_oracle(s)[2]
    assert imm[1:256].any()
    k = 1 + int(np.argmax(imm[1:256]))
    for slot in (0, 256):
        for key in ("pos", "old", "pe", "oe"):
            s[key][slot] = s[key][k]
    assert fe_oracle(s)[2][[0, 256]].all()
    fe_check_all(gpu_ctx, [s])
    for axis in (0, 1):
        dummy = float(s["old"][k, axis])
        imm2 = fe_oracle(s, dummy=dummy)[2]
        assert not imm2[[0, k, 256]].any() and np.array_equal(np.delete(imm2, [0, k, 256]), np.delete(fe_oracle(s)[2], [0, k, 256]))
        out = fe_check_all(gpu_ctx, [s], dummy=dummy)
        assert not out["immobile"][0, 0] and not out["immobile"][0, 256]


@pytest.mark.parametrize("img", [(320, 240), (321, 241), (321, 240), (64, 49)])
def test_feature_eval_image_centre(gpu_ctx, img):
    """pix_trans rounds an odd dimension up; a set whose features all sit exactly on the centre has np.amax(quad) == 0 and a zero
    centre term."""
    rng = np.random.default_rng(48)
    tx, ty = eo.pix_trans(img)
    assert (tx, ty) == ((img[0] + img[0] % 2) / 2, (img[1] + img[1] % 2) / 2)
    s = fe_set(rng, 70, img=(max(img[0], 60), max(img[1], 60)))
    s["pos"][11] = [tx, ty]                                      # one feature on the centre: quad == 0, centre term w2
    c = fe_set(rng, 9)
    flow = c["pos"] - c["old"]
    c["pos"][:] = [tx, ty]; c["old"] = c["pos"] - flow
    assert np.all((c["pos"][:, 0] - tx) ** 2 + (c["pos"][:, 1] - ty) ** 2 == 0)
    fe_check_all(gpu_ctx, [s, c], img=img)


# ================================================================================================ d_split
def ds_oracle(x, thr):
    with np.errstate(invalid="ignore"):                          # inf - inf and NaN gaps are part of the cases
        return eo.d_split(x, thr)


def ds_check(ctx, sets, thr, stride=None, counts=None):
    """The sets as one batch (slots past a set's data hold -7: reading them would change the result) against eo.d_split."""
    B = len(sets)
    stride = max(max(len(x) for x in sets), 1) if stride is None else stride
    d = np.full((B, stride), -7.0)
    for k, x in enumerate(sets):
        d[k, :len(x)] = x
    cn = np.array([len(x) for x in sets], np.int32) if counts is None else np.asarray(counts, np.int32)
    srt, dif, ns = ctx.d_split(d, thr, counts=cn)
    for k, x in enumerate(sets):
        c = len(x)
        s, g, n = ds_oracle(x, thr)
        assert np.array_equal(srt[k, :c], s, equal_nan=True), (k, c)            # as values: the order of -0.0 and 0.0 is not promised
        assert np.array_equal(dif[k, :max(c - 1, 0)], g, equal_nan=True), (k, c)
        assert ns[k] == n, (k, c, ns[k], n)
        assert np.all(srt[k, c:] == 0) and np.all(dif[k, max(c - 1, 0):] == 0)   # past the count, and diff[count - 1]
    return ns


DS_SIZES = [0, 1, 2, 3, 255, 256, 257, 1000, 2048, 2049, 4096]


def test_d_split_sizes(gpu_ctx):
    rng = np.random.default_rng(51)
    sets = [rng.normal(1.0, 0.5, n) for n in DS_SIZES]
    ds_check(gpu_ctx, sets, 0.01, stride=4096)
    for x in sets[1:]:                                           # single-set calls (a stride of 0 is not a call: the empty set is a count)
        s, g, n = gpu_ctx.d_split(x, 0.01)
        rs, rg, rn = ds_oracle(x, 0.01)
        assert np.array_equal(s, rs) and np.array_equal(g, rg) and n == rn, len(x)
    # a count above the stride is clamped to it
    x = rng.normal(1.0, 0.5, 257)
    ds_check(gpu_ctx, [x, x[:100]], 0.01, stride=257, counts=[257 + 3, 100])


def test_d_split_orderings(gpu_ctx):
    rng = np.random.default_rng(52)
    sets = []
    for n in (257, 1000):
        x = rng.normal(1.0, 0.5, n)
        sets += [np.sort(x), np.sort(x)[::-1].copy(), np.full(n, 0.75), np.round(x, 1)]
        assert len(np.unique(np.round(x, 1))) < n // 4
    ds_check(gpu_ctx, sets, 0.1)


def test_d_split_infinities_and_nan(gpu_ctx):
    rng = np.random.default_rng(53)
    seven = np.array([3.0, np.nan, 1.0, -0.0, 0.0, np.inf, 1.0])
    assert ds_oracle(seven, 0.5)[2] == 3
    sets = [seven]
    for n in (3, 257, 1000, 2049, 4096):                         # 4096: no padding at all; 2049: almost half of the network is padding
        x = rng.normal(1.0, 0.5, n)
        inf = x.copy(); inf[rng.choice(n, 3, replace=False)] = [np.inf, -np.inf, np.inf]
        one = x.copy(); one[n // 2] = np.nan
        few = inf.copy(); few[rng.choice(n, min(n, 40) // 2, replace=False)] = np.nan
        sets += [inf, one, few, np.full(n, np.nan)]
        assert np.isnan(ds_oracle(one, 0.3)[0][-1]) and np.isnan(ds_oracle(one, 0.3)[1][-1])
        assert ds_oracle(np.full(n, np.nan), 0.3)[2] == 0
    ns = ds_check(gpu_ctx, sets, 0.3, stride=4096)
    assert ns[0] == 3
    s, g, n = gpu_ctx.d_split(seven, 0.5)                        # the same as a single set (padded to 8)
    assert np.array_equal(s, [0.0, 0.0, 1.0, 1.0, 3.0, np.inf, np.nan], equal_nan=True) and n == 3
    assert np.array_equal(g, [0.0, 1.0, 0.0, 2.0, np.inf, np.nan], equal_nan=True)


def test_d_split_threshold(gpu_ctx):
    rng = np.random.default_rng(54)
    x = rng.integers(0, 200, 300).astype(np.float64)             # integer data: the gaps are exact, many equal the threshold
    gaps = np.diff(np.sort(x))
    assert (gaps == 1.0).sum() > 20 and (gaps == 0.0).sum() > 20 and (gaps == 2.0).sum() > 5
    for thr, want in ((1.0, int((gaps >= 1).sum())), (2.0, int((gaps >= 2).sum())), (0.0, 299), (np.inf, 0)):
        assert ds_oracle(x, thr)[2] == want
        assert ds_check(gpu_ctx, [x, x[:257]], thr)[0] == want
    y = x.copy(); y[17] = np.inf; y[200] = -np.inf               # an infinite gap reaches an infinite threshold (inf >= inf)
    assert ds_oracle(y, np.inf)[2] == 2
    assert ds_check(gpu_ctx, [y], np.inf)[0] == 2


# ================================================================================================ Kalman filter
def ld_kf(x, P, F, Q, Bm, u, H, Rm, z):
    """eo.kf_predict + eo.kf_correct restated in np.longdouble (Gauss-Jordan with partial pivoting for the solve): the yardstick
    for the float64 oracle's own error."""
    L = np.longdouble
    x, P, F, Q, H, Rm, z = [np.asarray(a, L) for a in (x, P, F, Q, H, Rm, z)]
    x = F @ x
    if Bm is not None and u is not None:
        x = x + np.asarray(Bm, L) @ np.asarray(u, L)
    P = F @ P @ F.T + Q
    S = H @ P @ H.T + Rm
    Y = H @ P
    A = np.concatenate([S, Y], axis=1)
    nm = len(S)
    for c in range(nm):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        A[[c, p]] = A[[p, c]]
        A[c] = A[c] / A[c, c]
        for r in range(nm):
            if r != c:
                A[r] = A[r] - A[r, c] * A[c]
    K = A[:, nm:].T
    x = x + K @ (z - H @ x)
    P = P - K @ H @ P
    return x, P


def kf_case(rng, ns, nm, nc, batch, R=None, p_scale=1.0):
    F = np.eye(ns) + 0.05 * rng.normal(size=(ns, ns)); H = rng.normal(size=(nm, ns)); Q = 0.01 * np.eye(ns)
    if R is None:
        A = rng.normal(size=(nm, nm)); R = A @ A.T + np.eye(nm)
    Bm = rng.normal(size=(ns, nc)) if nc else None
    x = rng.normal(size=(batch, ns))
    Bs = rng.normal(size=(batch, ns, ns)); P = p_scale * (Bs @ Bs.transpose(0, 2, 1) + np.eye(ns))
    u = rng.normal(size=(batch, nc)) if nc else None
    z = rng.normal(size=(batch, nm))
    return dict(F=F, H=H, Q=Q, R=R, B=Bm, x=x, P=P, u=u, z=z)


def kf_innovation_cov(k, b):
    Pp = k["F"] @ k["P"][b] @ k["F"].T + k["Q"]
    return k["H"] @ Pp @ k["H"].T + k["R"]


def kf_check(ctx, k, check_ld=True):
    """One composed predict + correct call against the oracle, filter by filter, at the tolerances of
    test_kf_reference_matrices_and_6_state (x 1e-11; P 1e-10 relative, 1e-12 absolute).  cond(S) < 1e4 is a condition on the
    inputs; with it the float64 oracle itself stays inside the same tolerances of its longdouble restatement (asserted)."""
    batch = len(k["x"])
    gx, gP = ctx.kf_predict_update(k["F"], k["H"], k["Q"], k["R"], k["x"], k["P"], B=k["B"], u=k["u"], z=k["z"])
    for b in range(batch):
        assert np.linalg.cond(kf_innovation_cov(k, b)) < 1e4
        ub = None if k["u"] is None else k["u"][b]
        xr, Pr = eo.kf_predict(k["x"][b], k["P"][b], k["F"], k["Q"], k["B"], ub)
        xr, Pr = eo.kf_correct(xr, Pr, k["H"], k["R"], k["z"][b])
        if check_ld and b < 4:
            xl, Pl = ld_kf(k["x"][b], k["P"][b], k["F"], k["Q"], k["B"], ub, k["H"], k["R"], k["z"][b])
            close(xr, xl.astype(np.float64), rtol=1e-11); close(Pr, Pl.astype(np.float64), rtol=1e-10, atol=1e-12)
        close(gx[b], xr, rtol=1e-11); close(gP[b], Pr, rtol=1e-10, atol=1e-12)
    return gx, gP


@pytest.mark.parametrize("ns", [1, 2, 3, 4, 6])
def test_kf_dimension_grid(gpu_ctx, ns):
    rng = np.random.default_rng(60 + ns)
    for nm in (1, 2, 3, 6):
        for nc in (0, 1, 3, 6):
            kf_check(gpu_ctx, kf_case(rng, ns, nm, nc, 5))


@pytest.mark.parametrize("batch", [1, 63, 64, 65, 200])
def test_kf_batches_across_the_block(gpu_ctx, batch):
    rng = np.random.default_rng(70)
    kf_check(gpu_ctx, kf_case(rng, 6, 3, 3, batch))
    kf_check(gpu_ctx, kf_case(rng, 3, 6, 1, batch))


@pytest.mark.parametrize("nm", [3, 6])
def test_kf_pivot_search_swaps_rows(gpu_ctx, nm):
    """R built from the SPD block [[1, 2], [2, 5]] (|s10| > s00) and a small P: the innovation covariance keeps its column maxima
    below the diagonal, so the Gauss-Jordan pivot search swaps rows; the result is np.linalg.solve's."""
    rng = np.random.default_rng(80 + nm)
    R = np.eye(nm)
    for i in range(0, nm - 1, 2 if nm == 6 else nm):
        R[i:i + 2, i:i + 2] = [[1.0, 2.0], [2.0, 5.0]]
    R *= 10.0
    assert np.all(np.linalg.eigvalsh(R) > 0) and abs(R[1, 0]) > R[0, 0]
    k = kf_case(rng, 6, nm, 3, 65, R=R, p_scale=0.002)
    for b in range(65):
        S = kf_innovation_cov(k, b)
        assert np.max(np.abs(S[1:, 0])) > abs(S[0, 0])           # the very first pivot is found below the diagonal
    kf_check(gpu_ctx, k)


def test_kf_split_calls_and_optional_control(gpu_ctx):
    rng = np.random.default_rng(90)
    k = kf_case(rng, 6, 3, 3, 65)
    gx, gP = kf_check(gpu_ctx, k)
    a = (k["F"], k["H"], k["Q"], k["R"])
    px, pP = gpu_ctx.kf_predict_update(*a, k["x"], k["P"], B=k["B"], u=k["u"], z=None)
    for b in range(65):
        xr, Pr = eo.kf_predict(k["x"][b], k["P"][b], k["F"], k["Q"], k["B"], k["u"][b])
        close(px[b], xr, rtol=1e-11); close(pP[b], Pr, rtol=1e-10, atol=1e-12)
    cx, cP = gpu_ctx.kf_predict_update(*a, px, pP, z=k["z"], do_predict=False)
    close(cx, gx, rtol=1e-13); close(cP, gP, rtol=1e-13)          # the split of test_kf_reference_matrices_and_6_state, at batch 65
    # B without u, and no B at all: no control term
    nx, nP = gpu_ctx.kf_predict_update(*a, k["x"], k["P"], B=k["B"], u=None, z=k["z"])
    mx, mP = gpu_ctx.kf_predict_update(*a, k["x"], k["P"], z=k["z"])
    assert np.array_equal(nx, mx) and np.array_equal(nP, mP)
    for b in range(65):
        xr, Pr = eo.kf_predict(k["x"][b], k["P"][b], k["F"], k["Q"], k["B"], None); xr, Pr = eo.kf_correct(xr, Pr, k["H"], k["R"], k["z"][b])
        close(nx[b], xr, rtol=1e-11); close(nP[b], Pr, rtol=1e-10, atol=1e-12)
    assert not np.allclose(nx, gx)


def test_kf_filters_are_independent(gpu_ctx):
    """20 steps of 65 filters whose inputs depend on the filter; the last one (alone in the second block) equals a single-filter run
    of the same inputs bit for bit - one thread runs one filter with the same instructions either way - and every step of it is
    the oracle's step from the same state."""
    rng = np.random.default_rng(91)
    k = kf_case(rng, 6, 3, 3, 65)
    a = (k["F"], k["H"], k["Q"], k["R"])
    x, P = k["x"], k["P"]
    xs, Ps = x[64].copy(), P[64].copy()
    for _ in range(20):
        u = rng.normal(size=(65, 3)) + np.arange(65)[:, None] * 0.01; z = rng.normal(size=(65, 3)) + np.arange(65)[:, None] * 0.02
        xr, Pr = eo.kf_predict(x[64], P[64], k["F"], k["Q"], k["B"], u[64]); xr, Pr = eo.kf_correct(xr, Pr, k["H"], k["R"], z[64])
        x, P = gpu_ctx.kf_predict_update(*a, x, P, B=k["B"], u=u, z=z)
        xs, Ps = gpu_ctx.kf_predict_update(*a, xs, Ps, B=k["B"], u=u[64:65], z=z[64:65])
        xs, Ps = xs.reshape(6), Ps.reshape(6, 6)
        close(x[64], xr, rtol=1e-11); close(P[64], Pr, rtol=1e-10, atol=1e-12)
    assert np.array_equal(x[64], xs) and np.array_equal(P[64], Ps)


# ================================================================================================ IMU and post-solve
def imu_msgs(rng, shape, secs0=1000):
    """Messages [..., 15]: small rotations and an acceleration with a steady offset from gravity, so that neither an increment nor
    a sum of increments cancels (the tolerances are the golden test's)."""
    m = np.zeros(shape + (15,))
    q = np.concatenate([0.05 * rng.normal(size=shape + (3,)), np.ones(shape + (1,))], axis=-1)
    m[..., 2:6] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    m[..., 6:9] = rng.normal(0, 0.2, shape + (3,)); m[..., 9:12] = rng.uniform(0.001, 0.01, shape + (3,))
    m[..., 12:15] = rng.normal(0, 0.3, shape + (3,)) + [3.0, -2.0, 4.0]
    m[..., 0] = secs0; m[..., 1] = rng.integers(0, 10 ** 9, shape)
    return m


def imu_dict(st):
    return dict(vel=st[0:3].copy(), old_time=float(st[3]), time_zero=st[4], first=bool(st[5] != 0.0))


def imu_vector(d):
    """The oracle's state in the device's layout (OFK_IMU_STATE), the `first` flag included."""
    return np.concatenate([d["vel"], [d["old_time"], d["time_zero"], 1.0 if d["first"] else 0.0], np.asarray(d["rotation"]).reshape(9), d["normal"],
                           d["ang"], d["ang_err"]])


def imu_oracle_step(d, m):
    return eo.imu_step(d, m[0], m[1], m[2:6], m[6:9], m[9:12], m[12:15])


@pytest.mark.parametrize("batch", [1, 64, 65, 130])
def test_imu_propagate_batches(gpu_ctx, ofk, batch):
    rng = np.random.default_rng(100 + batch)
    st = np.zeros((batch, ofk.IMU_STATE))
    st[:, 0:3] = rng.normal(0, 1.0, (batch, 3)) + [1.0, -2.0, 0.5]
    st[:, 5] = (np.arange(batch) % 3 == 1)                       # the first-message flag, mixed across the batch
    st[:, 3] = np.where(st[:, 5] == 0, rng.uniform(0, 2.0, batch), 0.0); st[:, 4] = np.where(st[:, 5] == 0, 1000 - 3, 0)
    msg = imu_msgs(rng, (batch,))
    msg[:, 0] += np.arange(batch) % 4                            # 3 .. 6 s since time_zero
    assert batch == 1 or (st[:, 5].any() and not st[:, 5].all())
    got = gpu_ctx.imu_propagate(st, msg)
    want = np.stack([imu_vector(imu_oracle_step(imu_dict(st[b]), msg[b])) for b in range(batch)])
    assert np.all(got[:, 5] == 0)
    close(got, want, rtol=1e-13, atol=1e-15)
    moved = st[:, 5] == 0
    assert np.all(got[moved, 0:3] != st[moved, 0:3]) and np.array_equal(got[~moved, 0:3], st[~moved, 0:3])


@pytest.fixture(scope="module")
def wide_ctx(ofk):
    """The resident IMU state lives in the context: 72 streams of tiny frames."""
    c = ofk.Context(0, 64, 64, 72, 16, 1)
    yield c
    c.close()


def test_imu_push_ragged_counts(wide_ctx, ofk):
    """imu_reset + imu_push + imu_state over 70 streams (two blocks of 64): counts 0 .. 5 of M = 5, one above M (clamped), one
    negative (none); time stamps that cross a seconds boundary; state and accumulated dv against a loop of eo.imu_step."""
    rng = np.random.default_rng(110)
    B, M = 70, 5
    s0 = np.zeros(ofk.IMU_STATE); s0[0:3] = [0.4, -0.3, 0.2]; s0[5] = 1.0
    msgs = imu_msgs(rng, (B, M))
    t0 = 0.80 + 0.002 * np.arange(B)[:, None] + 0.06 * np.arange(M)[None, :]      # 0.80 .. 1.18 s after secs0: secs steps, nsecs wraps
    msgs[..., 0] = 1000 + np.floor(t0); msgs[..., 1] = np.round((t0 - np.floor(t0)) * 1e9)
    assert np.all(msgs[:, 0, 0] == 1000) and np.all(msgs[:, -1, 0] == 1001) and np.all(msgs[:, -1, 1] < msgs[:, 0, 1])
    counts = (np.arange(B) % (M + 1)).astype(np.int32)
    counts[68] = M + 4; counts[69] = -2
    used = np.clip(counts, 0, M)
    assert set(used) == set(range(M + 1)) and used[68] == M and used[69] == 0 and used[64:].max() > 1
    wide_ctx.imu_reset(B, s0)
    wide_ctx.imu_push(msgs, counts)
    got, dv = wide_ctx.imu_state(B)
    more = imu_msgs(rng, (B, 1)); more[..., 0] = 1002              # a second push continues from the resident state and keeps accumulating
    wide_ctx.imu_push(more)
    got2, dv2 = wide_ctx.imu_state(B)
    for b in range(B):
        d = imu_dict(s0); acc = np.zeros(3)
        if used[b] == 0:
            assert np.array_equal(got[b], s0) and np.all(dv[b] == 0)
        for k in range(used[b] + 1):
            m = msgs[b, k] if k < used[b] else more[b, 0]
            new = imu_oracle_step(d, m)
            if not d["first"]:                                   # the increment imu_step adds to vel, by its own expression
                acc = acc + new["rotation"] @ (m[12:15] - 9.81 * new["normal"]) * (new["old_time"] - d["old_time"])
            d = new
            if k == used[b] - 1:
                close(got[b], imu_vector(d), rtol=1e-13, atol=1e-15)
                close(dv[b], acc, rtol=1e-13, atol=1e-15)
                assert (used[b] > 1) == bool(np.any(dv[b] != 0))
        close(got2[b], imu_vector(d), rtol=1e-13, atol=1e-15)
        close(dv2[b], acc, rtol=1e-13, atol=1e-15)


def rotations(rng, n):
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.stack([eo.quat_to_rot(*qq) for qq in q])


@pytest.mark.parametrize("batch", [1, 64, 65, 130])
def test_post_solve_batches(gpu_ctx, batch):
    rng = np.random.default_rng(120 + batch)
    v = rng.normal(0, 2.0, (batch, 3)); R = rotations(rng, batch); ang = rng.normal(0, 0.5, (batch, 3)); off = rng.normal(0, 0.2, (batch, 3))
    got = gpu_ctx.post_solve(v, R, ang, off)
    want = np.stack([eo.post_solve(v[b], R[b], ang[b], off[b]) for b in range(batch)])
    close(got, want, rtol=1e-14)


# ================================================================================================ flow model and feasibility
@pytest.mark.parametrize("n", [1, 255, 256, 257, 600])
def test_flow_model_and_feasibility_across_the_block(gpu_ctx, ofk, n):
    """Three problems with their own parameters, n points each: one point, one short of a block, a block, one more, and several."""
    rng = np.random.default_rng(130 + n)
    B = 3
    x = rng.uniform(-0.5, 0.5, (B, n, 2)); v = rng.normal(0, 1, (B, 3)) + [1.0, -1.0, 0.5]; om = rng.normal(0, 0.2, (B, 3))
    d = rng.uniform(0.5, 3, B); nrm = rng.normal(0, 0.1, (B, 3)) + [0, 0, 1]; t = rng.normal(0, 0.1, (B, 3))
    got_t = gpu_ctx.flow_model(x, v, om, d, nrm, t); got = gpu_ctx.flow_model(x, v, om, d, nrm)
    flow = np.stack([eo.generate_test_data(x[b], v[b], om[b], d[b], nrm[b], t[b]) for b in range(B)])
    for b in range(B):
        close(got_t[b], flow[b]); close(got[b], eo.generate_test_data(x[b], v[b], om[b], d[b], nrm[b]))
    u = flow + rng.normal(0, 0.05, flow.shape)
    vq = v + rng.normal(0, 0.1, v.shape)
    if n > 1:
        u[1, n // 2] = 0.0                                       # r_tilde's zero guard: (r, d) = (1, 1)
    r, dd = gpu_ctx.feasibility(ofk.FEAS_RTILDE, x, u, nrm, vq, dist=d)
    for b in range(B):
        rr, rd = eo.r_tilde(x[b], u[b], nrm[b], vq[b], d[b])
        close(r[b], rr); close(dd[b], rd)
    if n > 1:
        assert r[1, n // 2] == 1.0 and dd[1, n // 2] == 1.0
        u[1, n // 2] = flow[1, n // 2]                           # the legacy form has no guard
    r, dd = gpu_ctx.feasibility(ofk.FEAS_LEGACY, x, u, nrm, vq)
    for b in range(B):
        x3 = np.concatenate([x[b], np.ones((n, 1))], 1); u3 = np.concatenate([u[b], np.zeros((n, 1))], 1)
        rr, rd = eo.r_tilde_legacy(x3, u3, nrm[b], vq[b])
        close(r[b], rr); close(dd[b], rd)
    r, dd = gpu_ctx.feasibility(ofk.FEAS_SIM, x, u, nrm, vq, omega=om, t=t)
    for b in range(B):
        par, length = eo.feasibility_sim(x[b], vq[b], u[b], om[b], t[b], nrm[b])
        close(r[b], par); close(dd[b], length)
    r1, d1 = gpu_ctx.feasibility(ofk.FEAS_SIM, x[2], u[2], nrm[2], vq[2], omega=om[2], t=t[2])      # a single problem is the batch's row
    assert np.array_equal(r1, r[2]) and np.array_equal(d1, dd[2])


# ================================================================================================ refused inputs
def test_associate_sensors_refuses_non_finite_times_and_ranges(gpu_ctx, ofk):
    """np.argmin over distances that are all inf or NaN names no nearest sample: refused on the host, nothing is launched."""
    t_img = np.array([0.5, 1.5, 2.5]); imu_t = np.linspace(0, 3, 300); hgt_t = np.linspace(0, 3, 40); hgt_r = np.full(40, 1.2)
    q = np.tile([[0, 0, 0, 1.0]], (300, 1)); w = np.zeros((300, 3))
    for bad in (np.nan, np.inf, -np.inf):
        for which, at in (("t_img", 1), ("imu_t", 299), ("hgt_t", 0), ("hgt_r", 39)):
            arrs = dict(t_img=t_img.copy(), imu_t=imu_t.copy(), hgt_t=hgt_t.copy(), hgt_r=hgt_r.copy())
            arrs[which][at] = bad
            with pytest.raises(ofk.OfkError):
                gpu_ctx.associate_sensors(arrs["t_img"], arrs["imu_t"], q, w, arrs["hgt_t"], arrs["hgt_r"])
    _, ii, hi = gpu_ctx.associate_sensors(t_img, imu_t, q, w, hgt_t, hgt_r)     # the finite call still runs
    oi, oh, *_ = eo.associate(t_img, imu_t, q, w, hgt_t, hgt_r)
    assert np.array_equal(ii, oi) and np.array_equal(hi, oh)


def test_hist_overlap_refuses_non_finite_samples(gpu_ctx, ofk):
    """np.histogram raises ValueError on a non-finite range; the device refuses the sample on the host."""
    a = np.linspace(0, 1, 300); b = np.linspace(0.5, 2, 70)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            eo.overlap(np.append(a, bad), b)
        for x, y in ((np.append(a, bad), b), (a, np.insert(b, 0, bad))):
            with pytest.raises(ofk.OfkError):
                gpu_ctx.hist_overlap(x, y)
    assert gpu_ctx.hist_overlap(a, b) == eo.overlap(a, b)
