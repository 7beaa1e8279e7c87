"""GPU: the velocity solve (csrc/k_estimate.hip: solve_from_acc and its callers) where the suite had never taken it - ill-conditioned
clusters, the rank cut's two sides, single and coincident points, f32 pixel neighbours, and non-finite sensor values - against
tests/estimation_edge_cases.py: an exact rational solution of the same normal equations, lstsq truncated at the device's rank, and
the rule of include/ofk.h ("non-finite sums": rank 0, v = s = 0, residual 0, not solved, the filter at its prediction).

Every bound comes from estimation_edge_cases.py, where it is derived and measured on the numpy restatement; nothing here is set by what
the device returns.  The device's worst err / (kappa^2 eps |v|) per variant is printed by test_ladder (it is a report, not a bound)."""
import numpy as np
import pytest

import estimation_edge_cases as ec
import robust_reference as rr
from oracle import estimation_oracle as eo
from stream_oracle import NodeLoop, imu_messages

pytestmark = pytest.mark.gpu

WORST = {}                                                       # variant -> the device's worst ratio over the ladder so far


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ 1. the ladder
def check_rung(tag, out, p):
    ex = p["exact"]
    assert np.all(np.isfinite(out)), (tag, out)
    assert out[4] == 3, (tag, "rank", out[4], p["kappa"])
    v = out[:3] + ec.lever(p)                                    # the solve's own v: the entry took omega x t off
    err = np.linalg.norm(v - ex.v)
    ratio = err / (p["kappa"] ** 2 * ec.EPS * np.linalg.norm(ex.v))
    WORST[p["variant"]] = max(WORST.get(p["variant"], 0.0), ratio)
    r = ex.rss(v)
    print(f"{tag}: kappa {p['kappa']:.3e} err/(kappa^2 eps |v|) {ratio:.3f} s2 rel {abs(out[7] - p['s'][2]) / p['s'][2]:.2e} "
          f"rss {out[3]:.6e} exact {r:.6e} bound {ec.rss_bound(r, ex.bb):.2e}")
    assert err <= ec.v_bound(p["kappa"], ex.v), (tag, "v", err, ec.v_bound(p["kappa"], ex.v))
    assert np.all(np.abs(out[5:8] - p["s"]) <= ec.s_bound(p["kappa"], p["s"])), (tag, "s", out[5:8], p["s"])
    assert abs(out[3] - r) <= ec.rss_bound(r, ex.bb), (tag, "rss", out[3], r, ec.rss_bound(r, ex.bb))


@pytest.mark.parametrize("n", ec.COUNTS)
@pytest.mark.parametrize("variant", ec.VARIANTS)
def test_ladder(gpu_ctx, variant, n):
    probs = ec.ladder(variant, n)
    x = np.stack([p["x"] for p in probs]); u = np.stack([p["u"] for p in probs])
    kw = ec.solve_kwargs(variant, probs)
    out = gpu_ctx.velocity_solve(variant, x, u, **kw)
    for p, o in zip(probs, out):
        check_rung(f"variant {variant} n {n} h {p['h']}", o, p)
    # the same rungs under a valid mask among slots that hold NaN: the same bounds, and no trace of the NaN
    rng = np.random.default_rng(n)
    slots = 2 * n + 3
    X = np.full((len(probs), slots, 2), np.nan); U = np.full((len(probs), slots, 2), np.nan); valid = np.zeros((len(probs), slots), np.uint8)
    if variant == ec.OFMODULE:
        W = np.full((len(probs), slots), np.nan)
    for b, p in enumerate(probs):
        at = np.sort(rng.permutation(slots)[:n])
        X[b, at] = p["x"]; U[b, at] = p["u"]; valid[b, at] = 1
        if variant == ec.OFMODULE:
            W[b, at] = p["wgt"]
    if variant == ec.OFMODULE:
        kw["wgt"] = W
    out2 = gpu_ctx.velocity_solve(variant, X, U, valid=valid, **kw)
    for p, o in zip(probs, out2):
        check_rung(f"variant {variant} n {n} h {p['h']} masked", o, p)
    print(f"device worst err / (kappa^2 eps |v|) so far: {WORST}")


# ------------------------------------------------------------------------------------------------ 2. the rank window, degenerate sets
@pytest.mark.parametrize("n", ec.WINDOW_COUNTS)
def test_rank_window(gpu_ctx, n):
    probs = [ec.window_case(n, f) for f in ec.WINDOW_FACTORS]
    out = gpu_ctx.velocity_solve(ec.NODE, np.stack([p["x"] for p in probs]), np.stack([p["u"] for p in probs]), **ec.solve_kwargs(ec.NODE, probs))
    for p, o in zip(probs, out):
        ref = dict(rank=ec.expected_rank(p["kappa"], n), kappa=p["kappa"], v2=ec.lstsq_truncated(p["A"], p["B"], 2)[0], v3=None)
        assert ref["rank"] == (3 if p["factor"] < 1 else 2)
        rank = ec.check_solution(f"window n {n} kappa/thr {p['factor']}", o, ref, p["exact"])
        print(f"window n {n} kappa/thr {p['kappa'] / ec.thr(n):.4f}: rank {rank}, lambda_3/tol {(o[7] / o[5]) ** 2 / (ec.EPS * max(3 * n, 3)):.3e}")


@pytest.mark.parametrize("name", ("single", "identical_2", "identical_5", "identical_300", "f32_pairs"))
def test_degenerate_sets(gpu_ctx, name):
    st = ec.degenerate_sets()[name]
    B, n, _ = st["x"].shape
    kw = dict(d=np.full(B, ec.TRUTH["d"]), nrm=np.tile(ec.TRUTH["nrm"], (B, 1)), omega=np.tile(ec.TRUTH["omega"], (B, 1)))
    for flow, u in st["flows"].items():
        out = gpu_ctx.velocity_solve(ec.NODE, st["x"], u, **kw)
        seen = {}; worst = 0.0
        for b in range(B):
            ref = ec.degenerate_reference(st["x"][b], u[b])
            if name != "f32_pairs":
                assert ref["rank"] == 2                          # n coincident points carry two independent equations
            rank = ec.check_solution(f"{name} {flow} {b}", out[b], ref)
            seen[rank] = seen.get(rank, 0) + 1
            lam = out[b, 5:8] ** 2
            if rank == 2 and lam[0] > 0:
                worst = max(worst, lam[2] / (lam[0] * ec.EPS * max(3.0 * n, 3.0)))
        print(f"{name} {flow}: ranks {seen}, largest lambda_3 / tol among the rank-2 ones {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 3. the robust stage entry
def test_robust_entry_with_coincident_and_neighbour_pairs(gpu_ctx, ofk):
    from test_gpu_robust import compare, run_device              # the comparison of tests/test_gpu_robust.py, unchanged
    p, valid, special, _ = ec.robust_entry_case()
    s = ec.ROBUST_SETTING
    i, j = ofk.robust_pairs(s["seed"], ec.ROBUST_PROBLEM, s["hypotheses"], ec.ROBUST_M)
    assert sum(frozenset((int(a), int(b))) in special for a, b in zip(i, j)) >= 4
    out, w, st = run_device(gpu_ctx, ofk, rr.NODE, [p], valid[None], s)
    ref = compare(rr.NODE, p, valid, s, ec.ROBUST_PROBLEM, out[0], w[0], st[0], "robust entry")
    assert st[0, 7] == 0 and st[0, 3] == ec.ROBUST_M and int(st[0, 4]) == int(ref["stats"][4])


# ------------------------------------------------------------------------------------------------ 4. non-finite values at the entries
BAD_INPUTS = ("d_nan", "d_inf", "omega_nan", "ndp_zero", "x_nan")
NF_N, NF_B, NF_BAD = 40, 4, 1


def nonfinite_batch(variant, bad):
    """(clean, dirty): velocity_solve's arguments for four good problems, and the same with problem 1 made bad."""
    rng = np.random.default_rng(40 + variant)
    x = rng.uniform(-0.45, 0.45, (NF_B, NF_N, 2)); x[:, :, 1] *= 0.75
    d = rng.uniform(0.8, 1.5, NF_B); om = rng.uniform(-0.004, 0.004, (NF_B, 3)); t = rng.uniform(-0.1, 0.1, (NF_B, 3))
    nrm = np.tile([0.03, -0.02, 1.0], (NF_B, 1)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    u = np.stack([eo.generate_test_data(x[b], rng.uniform(-0.005, 0.005, 3), om[b], d[b], nrm[b]) for b in range(NF_B)])
    u += rng.standard_normal(u.shape) * 1e-4
    valid = (rng.uniform(size=(NF_B, NF_N)) < 0.8).astype(np.uint8); valid[:, :10] = 1
    clean = dict(x=x, u=u, d=d, nrm=nrm, omega=om, t=t, valid=valid)
    dirty = {k: v.copy() for k, v in clean.items()}
    b = NF_BAD
    if bad == "d_nan":
        dirty["d"][b] = np.nan
    elif bad == "d_inf":
        dirty["d"][b] = np.inf
    elif bad == "omega_nan":
        dirty["omega"][b, 1] = np.nan
    elif bad == "ndp_zero":                                      # n = (1, 0, 0) and a valid point with x = 0: n.p is exactly 0
        dirty["nrm"][b] = [1.0, 0.0, 0.0]; dirty["x"][b, 5, 0] = 0.0
    elif bad == "x_nan":
        dirty["x"][b, 5, 1] = np.nan
    return clean, dirty


def nonfinite_cases():
    for variant in (ec.NODE, ec.SIM):
        for bad in BAD_INPUTS:
            if not (variant == ec.SIM and bad == "ndp_zero"):    # SIM multiplies by n.p: a zero there is a finite row of zeros
                yield pytest.param(variant, bad, id=f"variant{variant}-{bad}")


def run_entry(ctx, ofk, entry, variant, a):
    x, u = a["x"], a["u"]
    kw = {k: a[k] for k in ("d", "nrm", "omega", "t", "valid")}
    if entry == "plain":
        return (ctx.velocity_solve(variant, x, u, **kw),)
    if entry == "robust":
        return ctx.velocity_solve_robust(variant, x, u, robust=ofk.robust_setting("tukey", hypotheses=16, iters=3, seed=5), **kw)
    if entry == "joint":
        return ctx.velocity_solve_joint(variant, x, u, **NF_SECOND["joint"], **kw)
    if entry == "plane":
        return ctx.velocity_solve_plane(variant, x, u, **NF_SECOND["plane"], **kw)
    if entry == "epi":
        return ctx.velocity_solve_epipolar(variant, x, u, **NF_SECOND["epi"], **kw)
    return ctx.velocity_solve_cov(variant, x, u, cov=ofk.cov_setting("propagate", sigma_flow=1e-4, sigma_pos=1e-4, sigma_d=0.01, sigma_omega=1e-3,
                                                                     sigma_normal=1e-3), **kw)


# the second-stage settings of these runs: every one succeeds on the clean batch (the plane and epipolar gates are open)
NF_SECOND = dict(joint=dict(sigma_flow=1e-4, sigma_omega=1e-3), plane=dict(sigma_flow=1e-4, sigma_normal=0.05, sigma_max=np.inf),
                 epi=dict(anchor=np.inf, anchor_min=5, sigma_max=np.inf))


def second_stage_flag1(entry, variant, a, b):
    """The second-stage record of problem b behind a solve that did not solve (out = 0, rank 0), by the reference: flag 1 in the
    layout of include/ofk.h."""
    import epi_reference as er
    import joint_reference as jr
    import plane_reference as pr
    args = (a["x"][b], a["u"][b], a["d"][b], a["nrm"][b], a["omega"][b])
    kw = dict(v_s=np.zeros(3), rss_s=0.0, valid=a["valid"][b])
    if entry == "joint":
        return jr.joint_solve(variant, *args, 1e-4, (1e-3,) * 3, rank=0, **kw)
    if entry == "plane":
        return pr.plane_solve(variant, *args, 1e-4, 0.05, sigma_max=np.inf, rank=0, **kw)
    return er.epi_solve(*args, anchor=np.inf, anchor_min=5, sigma_max=np.inf, **kw)


@pytest.mark.parametrize("variant,bad", list(nonfinite_cases()))
@pytest.mark.parametrize("entry", ("plain", "robust", "cov", "joint", "plane", "epi"))
def test_nonfinite_values_at_the_stage_entries(gpu_ctx, ofk, entry, variant, bad):
    clean, dirty = nonfinite_batch(variant, bad)
    ref = run_entry(gpu_ctx, ofk, entry, variant, clean)
    got = run_entry(gpu_ctx, ofk, entry, variant, dirty)
    good = [b for b in range(NF_B) if b != NF_BAD]
    assert np.all(ref[0][:, 4] == 3) and all(np.all(np.isfinite(r)) for r in ref)
    for r, g in zip(ref, got):                                   # the good problems: the bits of the batch without the bad value
        assert np.array_equal(bits(r[good]), bits(g[good])), (entry, variant, bad)
    out = got[0][NF_BAD]
    assert np.array_equal(out, np.zeros(8)), (entry, variant, bad, out)       # rank 0, v = 0, s = 0, residual 0 (even with a lever arm)
    m = int(dirty["valid"][NF_BAD].sum())
    if entry == "robust":
        w, st = got[1][NF_BAD], got[2][NF_BAD]
        assert np.array_equal(w, dirty["valid"][NF_BAD].astype(np.float64)), (w, bad)       # not solved: the kept weights stay 1
        assert np.array_equal(st, [0.0, m, m, m, -1.0, 0.0, 0.0, 1.0]), st
    if entry == "cov":
        cv = got[1][NF_BAD]
        assert cv[13] == 1 and not np.delete(cv, 13).any(), cv    # void
    if entry in ("joint", "plane", "epi"):                       # flag 1 in the header's layout; the clean batch took the second stage
        assert np.all(ref[1][:, 10] == 0), (entry, variant, ref[1][:, 10])
        want = second_stage_flag1(entry, variant, dirty, NF_BAD)
        rec = got[1][NF_BAD]
        assert want["flag"] == 1 and rec[10] == 1 and rec[11] == m, (entry, variant, bad, rec)
        assert np.array_equal(bits(rec), bits(want["rec"])), (entry, variant, bad, rec, want["rec"])
        zero = dict(joint=[3, 4, 5] + list(range(12, 32)), plane=[4, 5] + list(range(12, 32)), epi=list(range(0, 6)) + list(range(12, 32)))[entry]
        assert not rec[zero].any() and not rec[6:10].any(), (entry, variant, bad, rec)
        if entry == "epi":
            assert got[2].shape == (NF_B, NF_N, 4) and not got[2][NF_BAD].any(), (variant, bad)


# ------------------------------------------------------------------------------------------------ 5. a rangefinder dropout in the resident paths
H5, W5, NF5, DROP_T, MINF5, RAD5 = 240, 320, 7, 3, 70, 12
OFFSET5 = (0.0, 0.0, 0.1)
_clips = {}


def clips():
    if not _clips:
        from of_amd import synth
        seqs = [synth.render_sequence(H5, W5, 500 + b, NF5, v=(0.004, -0.003, 0.002), omega=(0.0, 0.0, 0.004 * b), d=1.0) for b in range(2)]
        _clips["frames"] = np.stack([s[0] for s in seqs]); _clips["infos"] = [s[1] for s in seqs]
    return _clips["frames"], _clips["infos"]


def dropout_solver(loop, feas_T, min_cnt):
    """NodeLoop's solver plug for these runs: stream_oracle.plain_solve / feasibility_solve (the prior being the loop's dead-reckoned
    velocity at the time of the solve), which reports "not solved" for a non-finite d.  The keep flags do not depend on d."""
    def solve(x, u, ok, d, nrm, om):
        keep = np.array(ok, bool)
        if feas_T is not None and len(x):
            with np.errstate(all="ignore"):
                keep &= eo.r_tilde(x, u, nrm, np.asarray(loop[0].imu["vel"], np.float64), 1.0)[0] <= feas_T
        solved = bool(int(keep.sum()) > min_cnt and np.isfinite(d))
        return dict(v=eo.solve_lgs_node(x[keep], u[keep], d, nrm, om)[0] if solved else None, solved=solved, keep=keep)
    return solve


def stream_run(ofk, kind, drop):
    """Two streams, six steps; with `drop` stream 1's d is NaN at step DROP_T only.  Per step: rec, fused (None for the plain step),
    tracks, counts, filter state, IMU state."""
    from of_amd.pipeline import FlowStream, PipelineConfig, FusionConfig, FilterModel
    frames, infos = clips()
    cfg = PipelineConfig(max_corners=90, quality=0.04, min_distance=9, block_size=7, win=15, max_level=2, max_count=20, eps=0.03)
    fusion = None
    if kind in ("filter", "filter_robust"):
        fusion = FusionConfig(filter=True, control=ofk.CONTROL_SENSORS, z_sign=1.0, z_source=1, min_solve=2, model=FilterModel.kf3())
        if kind == "filter_robust":
            cfg.robust = "tukey"; cfg.robust_hypotheses = 16; cfg.robust_iters = 3
    elif kind == "imu":
        fusion = FusionConfig.node()
        cfg.use_feasibility = True; cfg.feas_T = 2.0             # r_tilde is a cosine: every point passes while the prior velocity is finite
    sensors = np.concatenate([ofk.make_sensors(1, d=i["d"], normal=i["n"], omega=i["omega"], offset=OFFSET5, scaling=i["scaling"], cx=i["cx"], cy=i["cy"])
                              for i in infos])
    fs = FlowStream(W5, H5, batch=2, cfg=cfg, min_features=MINF5, mask_radius=RAD5, fusion=fusion)
    steps = []
    try:
        tracks, counts = fs.begin(frames[:, 0])
        first = (tracks.copy(), counts.copy())
        rng = np.random.default_rng(5)
        for t in range(1, NF5):
            sr = sensors.copy()
            if drop and t == DROP_T:
                sr[1, 0] = np.nan
            msgs = np.stack([imu_messages(rng, 100.0 + 0.1 * t + 7 * b, 3) for b in range(2)])
            if kind == "imu":
                fs.push_imu(msgs)
            if fusion is None:
                rec, tracks, counts = fs.step(frames[:, t], sr); fused = None
            else:
                rec, fused, tracks, counts = fs.step_fused(frames[:, t], sr)
            steps.append(dict(rec=rec.copy(), fused=None if fused is None else fused.copy(), tracks=tracks.copy(), counts=counts.copy(), sr=sr, msgs=msgs,
                              filt=fs.ctx.filter_state(2) if fusion is not None and fusion.filter else None,
                              imu=fs.ctx.imu_state(2)[0] if kind == "imu" else None))
    finally:
        fs.close()
    return first, steps, cfg, fusion


@pytest.mark.parametrize("kind", ("step", "filter", "imu", "filter_robust"))
def test_rangefinder_dropout_in_a_resident_stream(pkg, ofk, kind):
    frames, infos = clips()
    first, clean, cfg, fusion = stream_run(ofk, kind, drop=False)
    _, steps, _, _ = stream_run(ofk, kind, drop=True)
    for k, (a, b) in enumerate(zip(clean, steps)):               # stream 0 never hears of it
        assert np.array_equal(bits(a["rec"][0]), bits(b["rec"][0])) and a["counts"][0] == b["counts"][0], k
        assert np.array_equal(a["tracks"][0].view(np.uint32), b["tracks"][0].view(np.uint32)), k
        if a["fused"] is not None:
            assert np.array_equal(bits(a["fused"][0]), bits(b["fused"][0])), k
        if a["filt"] is not None:
            assert np.array_equal(bits(a["filt"][0][0]), bits(b["filt"][0][0])) and np.array_equal(bits(a["filt"][1][0]), bits(b["filt"][1][0])), k
        if a["imu"] is not None:
            assert np.array_equal(bits(a["imu"][0]), bits(b["imu"][0])), k
    loop = None
    if kind != "filter_robust":                                  # stream 1 against the node's loop with the dropout plug
        holder = []
        loop = NodeLoop(frames[1, 0], cfg, MINF5, RAD5, solve=dropout_solver(holder, 2.0 if kind == "imu" else None, 2),
                        imu_offset=OFFSET5 if kind == "imu" else None, model=fusion.model if kind == "filter" else None, overwrite=kind == "imu")
        holder.append(loop)
        assert first[1][1] == len(loop.tracks) and np.array_equal(first[0][1, :first[1][1]], loop.tracks)
    for k, s in enumerate(steps):
        t = k + 1
        rec, fused = s["rec"][1], None if s["fused"] is None else s["fused"][1]
        assert np.all(np.isfinite(rec)), (t, rec)
        if t == DROP_T:                                          # the rule: rank 0, v = s = 0, residual 0, cnt as counted, not solved
            assert rec[4] == 0 and not rec[0:4].any() and not rec[5:8].any() and rec[15] == 0 and rec[11] >= 3 and rec[13] >= rec[11], rec
            if fused is not None:
                assert fused[7] == 0 and np.all(np.isfinite(fused))
        else:
            assert rec[4] == 3 and rec[11] >= 3, (t, rec)
            if fused is not None:
                assert rec[15] == 1 and fused[7] == 1 and np.all(np.isfinite(fused)), (t, fused)
        if s["filt"] is not None:
            assert np.all(np.isfinite(s["filt"][0][1])) and np.all(np.isfinite(s["filt"][1][1])), t
        if s["imu"] is not None:
            assert np.all(np.isfinite(s["imu"][1])), t
        if kind == "filter_robust" and t == DROP_T:              # the filter at its prediction: F = B = I, no control
            px, pP = steps[k - 1]["filt"][0][1], steps[k - 1]["filt"][1][1]
            m = fusion.model
            xp, Pp = eo.kf_predict(px, pP, m.F, m.Q, m.B, np.zeros(3))
            np.testing.assert_allclose(s["filt"][0][1], xp, rtol=1e-12, atol=1e-15); np.testing.assert_allclose(s["filt"][1][1], Pp, rtol=1e-12, atol=1e-18)
        if loop is None:
            continue
        o = loop.step(frames[1, t], s["sr"][1], s["msgs"][1] if kind == "imu" else ())
        assert o["solved"] == (t != DROP_T)
        n = int(s["counts"][1])
        assert n == len(o["tracks"]) and rec[12] == o["n_old"] and rec[13] == o["n_tracked"] and rec[11] == int(np.count_nonzero(o["keep"])), (t, rec[11:14])
        assert np.array_equal(s["tracks"][1, :n].view(np.uint32), o["tracks"].astype(np.float32).view(np.uint32)), t
        if o["solved"]:
            np.testing.assert_allclose(rec[:3], o["v"], rtol=1e-8, atol=1e-12)
            np.testing.assert_allclose(rec[8:11], o["v_uav"], rtol=1e-8, atol=1e-12)
        if kind == "filter":                                     # at DROP_T the loop did not correct: x, P are the prediction
            np.testing.assert_allclose(fused[:3], o["x"], rtol=1e-8, atol=1e-12)
            np.testing.assert_allclose(s["filt"][0][1], o["x"], rtol=1e-8, atol=1e-12); np.testing.assert_allclose(s["filt"][1][1], o["P"], rtol=1e-10, atol=1e-14)
        if kind == "imu":                                        # at DROP_T the loop did not overwrite: the dead-reckoned velocity stays
            np.testing.assert_allclose(fused[:3], o["vel"], rtol=1e-8, atol=1e-12)
            np.testing.assert_allclose(s["imu"][1, 0:3], o["vel"], rtol=1e-8, atol=1e-12)


@pytest.mark.parametrize("cov", (False, True))
def test_rangefinder_dropout_in_the_pair_filter(pkg, ofk, cov):
    from of_amd import synth
    from of_amd.pipeline import FlowPipeline, PipelineConfig, FilterModel
    B, bad = 3, 1
    pairs = [synth.render_pair(H5, W5, 30 + b, v=(0.004, -0.003, 0.002), omega=(0.003, -0.002, 0.004), d=1.0) for b in range(B)]
    prev = np.stack([p["prev"] for p in pairs]); nxt = np.stack([p["next"] for p in pairs])
    cfg = PipelineConfig(max_corners=100, quality=0.05, min_distance=8, block_size=7, win=15, max_level=2, max_count=20, eps=0.03)
    model = FilterModel.kf3(); model.R = 1e-4 * np.eye(3); model.P0 = 1e-4 * np.eye(3)
    results = []
    for drop in (False, True):
        sensors = np.concatenate([ofk.make_sensors(1, d=p["d"], normal=p["n"], omega=p["omega"], scaling=p["scaling"], cx=p["cx"], cy=p["cy"]) for p in pairs])
        if drop:
            sensors[bad, 0] = np.nan
        pipe = FlowPipeline(W5, H5, B, cfg)
        try:
            pipe.ctx.filter_configure(model, B)
            if cov:
                pipe.ctx.set_cov(mode="propagate", sigma_flow=0.05, sigma_pos=0.05, sigma_d=0.01, sigma_omega=1e-3, sigma_normal=1e-3, filter_r=True, r_floor=1e-8)
            pipe.upload(prev, nxt, sensors)
            out = pipe.run()
            pipe.ctx.pairs_filter_step(B, z_sign=-1.0, z_source=1)
            x, P = pipe.ctx.filter_state(B)
            results.append((out["records"].copy(), x.copy(), P.copy(), pipe.covariances().copy() if cov else None))
        finally:
            pipe.close()
    (rec0, x0, P0, cv0), (rec1, x1, P1, cv1) = results
    assert np.all(rec0[:, 4] == 3) and np.all(np.isfinite(x0))
    for b in range(B):
        if b != bad:                                             # the others are untouched
            assert np.array_equal(bits(rec0[b]), bits(rec1[b])) and np.array_equal(bits(x0[b]), bits(x1[b])) and np.array_equal(bits(P0[b]), bits(P1[b]))
            assert not cov or (np.array_equal(bits(cv0[b]), bits(cv1[b])) and cv1[b, 13] == 0)
    r = rec1[bad]
    assert np.all(np.isfinite(r)) and r[4] == 0 and not r[0:4].any() and not r[5:8].any() and r[15] == 0 and r[11] == rec0[bad, 11] >= 3, r
    xp, Pp = eo.kf_predict(np.array(model.x0), np.array(model.P0), model.F, model.Q)
    np.testing.assert_allclose(x1[bad], xp, rtol=1e-12, atol=1e-15); np.testing.assert_allclose(P1[bad], Pp, rtol=1e-12, atol=1e-18)
    assert not np.allclose(x0[bad], xp, atol=1e-6)               # the clean run did correct
    if cov:                                                      # void record, the deferred correct skipped (no NIS, not gated)
        assert cv1[bad, 13] == 1 and not np.delete(cv1[bad], 13).any(), cv1[bad]
