"""The case table of the position filter's stage-entry test (tests/test_gpu_pos_filter.py (a)), kept apart so that a CPU test
(tests/test_pos_filter_cases.py) can show on the restatement that the table is not vacuous.

A script is one stream: dict(name, steps=[dict(v, solved, key, rw, inp)]).  A group is dict(name, setting, scripts): the scripts of one
group run as the streams of one batch under one setting.  Every script of a group has the same number of steps."""
import numpy as np

import pos_filter_reference as R

NAN, INF = float("nan"), float("inf")


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
    return q * np.sign(np.linalg.det(q))


def plain_step(rng, v=True, D=True, fix=True, clone=False, du=True):
    """One step whose three updates are attempted or not and that re-keys or not; every number drawn afresh."""
    A = rng.normal(0, 1, (3, 3))
    C_T = (A @ A.T + 0.5 * np.eye(3)) * 1e-6
    key = R.key_record(rng.normal(0, 0.01, 3), C_T, flag=0 if D else 1, reason=(2 if D else 1) if clone else 0)
    inp = np.zeros(R.INPUT)
    if du:
        inp[0:3] = rng.normal(0, 1e-3, 3)
    if fix:
        inp[3] = 1.0; inp[4:7] = rng.normal(0, 0.03, 3); inp[7:10] = rng.uniform(0.02, 0.08, 3)
    return dict(v=rng.normal(0, 0.01, 3), solved=1 if v else 0, key=key, rw=rotation(rng), inp=inp)


def combos(seed):
    """The 8 attempted / not attempted combinations of the updates x cloned or not x fresh or not on entry: a first step that leaves the
    stream fresh (it re-keys) or not (a displacement update without a re-key), then the step of the case."""
    rng = np.random.default_rng(seed)
    out = []
    for fresh in (1, 0):
        for clone in (0, 1):
            for m in range(8):
                v, D, fix = bool(m & 1), bool(m & 2), bool(m & 4)
                first = plain_step(rng, D=True, clone=bool(fresh))
                out.append(dict(name=f"fresh{fresh}-clone{clone}-v{int(v)}D{int(D)}f{int(fix)}", steps=[first, plain_step(rng, v, D, fix, bool(clone))]))
    return out


def broken(seed):
    """NaN / inf in each of v_uav, D, C_T, R_world, the fix and its sigma, in a step that would attempt all three updates."""
    rng = np.random.default_rng(seed)
    out = []
    for what in ("v", "D", "C_T", "rw", "fix", "sigma", "du"):
        for bad in (NAN, INF, -INF):
            s = plain_step(rng)
            k = int(rng.integers(0, 3))
            if what == "v":
                s["v"][k] = bad
            elif what == "D":
                s["key"][10 + k] = bad
            elif what == "C_T":
                s["key"][20 + int(rng.integers(0, 6))] = bad
            elif what == "rw":
                s["rw"][k, int(rng.integers(0, 3))] = bad
            elif what == "fix":
                s["inp"][4 + k] = bad
            elif what == "sigma":
                s["inp"][7 + k] = bad
            else:
                s["inp"][k] = bad
            out.append(dict(name=f"{what}={bad}", steps=[plain_step(rng, clone=True), s]))
    for k in range(3):                                           # a sigma of zero or below: the fix is not attempted
        s = plain_step(rng)
        s["inp"][7 + k] = 0.0 if k else -0.05
        out.append(dict(name=f"sigma{k}<=0", steps=[plain_step(rng), s]))
    return out


def outliers(seed):
    """Under nis_max = 9: an innovation of tens of sigma in each update (gated), beside streams that pass."""
    rng = np.random.default_rng(seed)
    out = []
    for what in ("v", "D", "fix", "none"):
        a, b, c = plain_step(rng, clone=True, fix=False), plain_step(rng, fix=False), plain_step(rng)
        for s in (a, b, c):                                      # small innovations that pass ...
            s["v"] = rng.normal(0, 1e-4, 3); s["key"][10:13] = rng.normal(0, 1e-5, 3); s["inp"][0:3] = 0.0; s["inp"][4:7] = rng.normal(0, 1e-3, 3)
            s["inp"][3] = 1.0; s["inp"][7:10] = 0.05
        if what == "v":                                          # ... but for the one that is tens of sigma out
            c["v"] = np.array([0.5, -0.5, 0.5])
        elif what == "D":
            c["key"][10:13] = [0.3, 0.3, -0.3]
        elif what == "fix":
            c["inp"][4:7] = [3.0, -3.0, 3.0]
        out.append(dict(name="gated-" + what, steps=[a, b, c]))
    return out


def degenerate(seed):
    """Nothing is uncertain (every prior and process noise 0, share 0, floor 0) and C_T = 0: S of the displacement is exactly 0 and the
    update is refused; the velocity's and the fix's S overflow with a sigma of 1e200 (finite, so they are attempted) and are refused."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(3):
        steps = []
        for t in range(2):
            s = plain_step(rng, clone=t == 0)
            s["key"][20:26] = 0.0
            s["inp"][7:10] = 1e200
            steps.append(s)
        out.append(dict(name=f"refused-{k}", steps=steps))
    return out


def sequence(seed, n, steps=8):
    """n streams over `steps` steps with a re-key in the middle and a fix on two of them."""
    rng = np.random.default_rng(seed)
    return [dict(name=f"seq{i}", steps=[plain_step(rng, v=t != 2, D=t != 5, fix=t in (3, 6), clone=t in (0, 4)) for t in range(steps)]) for i in range(n)]


BASE = dict(dt=0.8, sigma_v=2e-3, floor=2e-4, infl=1.3, share=0.5, q_p=1e-4, q_v=1e-3, q_b=1e-5, p0_p=0.05, p0_v=0.1, p0_b=1e-3)
PRIORS = (1e-4, 1e-2, 1.0, 1e2, 1e4, 1e6, 1e8)
SHARES = (0.0, 0.5, 1.0)


def groups():
    g = [dict(name="combos", setting=R.setting(**BASE), scripts=combos(11) + broken(12)),
         dict(name="gated", setting=R.setting(**dict(BASE, nis_max=9.0)), scripts=outliers(13)),
         dict(name="refused", setting=R.setting(dt=1.0, sigma_v=1e200, floor=0.0, infl=1.0, share=0.0, q_p=0.0, q_v=0.0, q_b=0.0, p0_p=0.0, p0_v=0.0,
                                                p0_b=0.0), scripts=degenerate(14)),
         dict(name="held-bias", setting=R.setting(**dict(BASE, p0_b=0.0, q_b=0.0)), scripts=sequence(15, 3))]
    g += [dict(name=f"share{s}", setting=R.setting(**dict(BASE, share=s)), scripts=sequence(20 + i, 3)) for i, s in enumerate(SHARES)]
    g += [dict(name=f"prior{p:g}", setting=R.setting(**dict(BASE, p0_p=p, p0_v=p, p0_b=p)), scripts=sequence(30 + i, 3)) for i, p in enumerate(PRIORS)]
    return g


def restate(group, pos0=(0.0, 0.0, 0.0)):
    """The restatement over a group -> per script the list of (state after the step, rec)."""
    out = []
    for sc in group["scripts"]:
        st = R.new_state(pos0)
        rows = []
        for s in sc["steps"]:
            rec = R.step(st, group["setting"], s["v"], s["solved"], s["key"], s["rw"], s["inp"])
            rows.append(({k: v.copy() for k, v in st.items()}, rec))
        out.append(rows)
    return out
