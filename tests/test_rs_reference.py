"""The rolling shutter on the CPU (tests/rs_reference.py, the numpy restatement of include/ofk.h): what the per-row capture time costs
the velocity solve and what the two corrections give back (the table in rs_reference's docstring is this module's print-out), the
analytic cases the arithmetic must reproduce, the fallback rule, and a rendered scene.

Bounds: the setting was specified with 0.25 x (gyro, all 18 cases) and 0.6 x (flow, time stamp at the frame's middle); the experiment gives at most
0.111 x and 0.366 x, so both keep a factor of two or more.  The analytic cases hold to 1e-12 in float64: the arithmetic is a handful
of operations on numbers of the size of 1 (normalised coordinates) or 1e3 (pixels: 1e3 * 2^-52 = 2e-13 per operation)."""
import numpy as np
import pytest

import batch_oracle as BO
import rs_reference as R

_table = {}


def table():
    if not _table:
        for name, m in R.MOTIONS.items():
            for a in R.ANCHORS:
                for ro in R.READOUTS:
                    _table[name, a, ro] = R.experiment(m, ro, a)
    return _table


def test_gyro_mode_gives_the_solve_back_in_all_18_cases():
    worst = 0.0
    for key, r in table().items():
        print(key, {k: round(v, 5) for k, v in r.items()})
        assert r["raw"] >= 0.005, (key, r)                       # there is something to correct
        assert r["gyro"] <= 0.25 * r["raw"], (key, r)
        worst = max(worst, r["gyro"] / r["raw"])
    print("largest gyro / raw", worst)


def test_flow_mode_helps_with_the_time_stamp_at_the_middle_row():
    worst = 0.0
    for (name, a, ro), r in table().items():
        if a == 0.5:
            assert r["flow"] <= 0.6 * r["raw"], (name, a, ro, r)
            worst = max(worst, r["flow"] / r["raw"])
        else:                                                    # recorded, not asserted: a straight line over up to 0.9 frame intervals
            print(name, a, ro, "flow / raw", round(r["flow"] / r["raw"], 3))
    print("largest flow / raw at anchor 0.5", worst)


def rotated(x, om, t):
    """P(t) = R(t om) P(0) under dP/dt = om x P, projected; x [N, 2], t [N]."""
    P = np.concatenate([x, np.ones((len(x), 1))], 1)
    out = np.empty_like(x)
    for i in range(len(x)):
        phi = om * t[i]; th = np.linalg.norm(phi)
        K = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]])
        Rm = np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / th ** 2) * K @ K if th > 0 else np.eye(3)
        q = Rm @ P[i]
        out[i] = q[:2] / q[2]
    return out


@pytest.mark.parametrize("readout,anchor", [(0.9, 0.5), (-0.9, 0.0), (0.5, 1.0)])
def test_pure_rotation_comes_back_to_the_time_stamps_in_gyro_mode(readout, anchor):
    """A point under pure rotation observed at ANY two row times: the caller's rows decide the times, whatever they are."""
    rng = np.random.default_rng(3)
    n, f, c, H = 200, 1000.0, np.array([640.0, 480.0]), 960
    om = np.array([0.02, -0.03, 0.15])
    x0 = rng.uniform(-0.5, 0.5, (n, 2)); x1 = rotated(x0, om, np.ones(n))          # at the two time stamps
    ideal0, ideal1 = x0 * f + c, x1 * f + c
    # the observation at its own row time, the row found by fixed-point iteration (the raw image is the ideal one here)
    obs = []
    for k, xs in ((0, x0), (1, x1)):
        t = np.zeros(n)
        for _ in range(40):
            p = rotated(xs, om, t) * f + c
            t = readout * (p[:, 1] / H - anchor)
        obs.append(rotated(xs, om, t) * f + c)
    sr = R.sensor_row(dict(omega=om), 1.0 / f, c[0], c[1])
    a, b, span, _ = R.correct_f64(R.rshutter(R.GYRO, readout, anchor, H), obs[0], obs[1], sensors=sr[None])
    assert np.abs(span - 1.0).max() > 0.01
    # 1e-12 of the normalised coordinates the arithmetic runs in = 1e-9 pixels at f = 1000
    assert np.abs((a - ideal0) / f).max() <= 1e-12 and np.abs((b - ideal1) / f).max() <= 1e-12, (np.abs(a - ideal0).max(), np.abs(b - ideal1).max())


@pytest.mark.parametrize("readout,anchor", [(0.9, 0.5), (-0.9, 0.0), (0.5, 1.0)])
def test_constant_image_velocity_comes_back_in_flow_mode(readout, anchor):
    rng = np.random.default_rng(4)
    n, H = 200, 960
    q0 = np.stack([rng.uniform(0, 1280, n), rng.uniform(0, 960, n)], -1); vel = rng.uniform(-60, 60, (n, 2))
    q1 = q0 + vel
    # p(t) = q0 + t vel; the row time of each observation solves t = readout ((q0.y + t vel.y) / H - anchor): linear in t
    t0 = readout * (q0[:, 1] / H - anchor) / (1.0 - readout * vel[:, 1] / H)
    t1 = readout * (q1[:, 1] / H - anchor) / (1.0 - readout * vel[:, 1] / H)
    r0, r1 = q0 + t0[:, None] * vel, q1 + t1[:, None] * vel
    a, b, _, _ = R.correct_f64(R.rshutter(R.FLOW, readout, anchor, H), r0, r1)
    assert np.abs(a - q0).max() <= 1e-12 * 1280 and np.abs(b - q1).max() <= 1e-12 * 1280, (np.abs(a - q0).max(), np.abs(b - q1).max())


def test_readout_zero_returns_the_input_bits_and_no_omega_is_flow_mode():
    rng = np.random.default_rng(5)
    p0 = np.stack([rng.uniform(0, 1280, (2, 300)), rng.uniform(0, 960, (2, 300))], -1).astype(np.float32)
    p1 = (p0 + rng.uniform(-40, 40, p0.shape)).astype(np.float32)
    p1[0, 7] = np.nan; p1[1, 9, 0] = 1e7                         # status-0 garbage comes out as it went in
    sr = np.stack([R.sensor_row(R.FAST, 1e-3, 640.0, 480.0), R.sensor_row(R.YAW, 1.1e-3, 600.0, 500.0)])
    for mode in (R.FLOW, R.GYRO):
        a, b = R.correct_points(R.rshutter(mode, 0.0, 0.3, 960), p0, p1, sensors=sr)
        assert np.array_equal(a.view(np.uint32), p0.view(np.uint32)) and np.array_equal(b.view(np.uint32), p1.view(np.uint32)), mode
    still = sr.copy(); still[:, 4:7] = 0.0
    ok = np.isfinite(p1).all(-1) & (np.abs(p1) < 1e6).all(-1)
    for ro in (0.9, -0.5):
        g = R.correct_f64(R.rshutter(R.GYRO, ro, 0.5, 960), p0, p1, sensors=still[:, None, :])
        f = R.correct_f64(R.rshutter(R.FLOW, ro, 0.5, 960), p0, p1)
        # 1e-12 relative to the pixel coordinates (up to 1280)
        assert np.abs(g[0][ok] - f[0][ok]).max() <= 1e-12 * 1280 and np.abs(g[1][ok] - f[1][ok]).max() <= 1e-12 * 1280


def test_fallback_rule():
    nan = np.nan
    rs = R.rshutter(R.FLOW, 0.9, 0.5, 960)
    p0 = np.array([[100.0, 900.0], [100.0, 100.0], [5.0, 5.0], [5.0, 5.0], [300.0, 400.0]], np.float32)
    p1 = np.array([[100.0, 100.0], [nan, 120.0], [1e7, 9.0], [6.0, 7.0], [310.0, 380.0]], np.float32)      # span 0.25 / NaN / 1e7 / fine / fine
    a, b, good = R.correct_points(rs, p0, p1, full=True)
    assert good.tolist() == [False, False, False, True, True]
    for i in range(3):
        assert np.array_equal(a[i].view(np.uint32), p0[i].view(np.uint32)) and np.array_equal(b[i].view(np.uint32), p1[i].view(np.uint32))
    assert np.isfinite(a[3:]).all() and not np.array_equal(a[4], p0[4])
    sr = R.sensor_row(R.SLOW, 0.0, 640.0, 480.0)                 # scaling 0: every point takes the fallback in gyro mode
    a, b, good = R.correct_points(dict(rs, mode=R.GYRO), p0, p1, sensors=sr[None], full=True)
    assert not good.any() and np.array_equal(a.view(np.uint32), p0.view(np.uint32)) and np.array_equal(b.view(np.uint32), p1.view(np.uint32))
    # with ideal points the fallback returns THOSE, and the rows come from the raw ones
    i0, i1 = p0 + np.float32(3.0), p1 + np.float32(2.0)
    a, b, good = R.correct_points(rs, p0, p1, i0, i1, full=True)
    assert good.tolist() == [False, False, False, True, True] and np.array_equal(a[0], i0[0]) and np.array_equal(b[2], i1[2])
    t0, t1, span = R.row_times(rs, p0, p1)
    assert np.allclose(a[4], i0[4] - t0[4] * (i1[4] - i0[4]).astype(np.float64) / span[4], atol=1e-4)


def test_rendered_scene_through_a_rolling_shutter(pkg):
    fr0, sr, cfg, _ = R.scene(0.0)
    fr, sr, cfg, rs = R.scene()
    e_gs = R.rel_err(BO.oracle_chain(fr0["prev"], fr0["next"], cfg, sr)["v"])
    chain = BO.oracle_chain(fr["prev"], fr["next"], cfg, sr)
    e_off, e_on = R.rel_err(chain["v"]), R.rel_err(R.solve_corrected(rs, chain, sr))
    e_flow = R.rel_err(R.solve_corrected(dict(rs, mode=R.FLOW), chain, sr))
    print("readout 0", e_gs, "gyro", e_on, "flow", e_flow, "uncorrected", e_off)
    assert e_off >= 3.0 * e_gs, (e_off, e_gs)
    # nearer to the global shutter's than to the uncorrected one: measured 0.0006 against 0.029, asserted with a factor of 4 in hand
    assert 4.0 * abs(e_on - e_gs) <= abs(e_off - e_on), (e_gs, e_on, e_off)


def test_synth_without_a_rolling_shutter_is_what_it_was(pkg):
    """rolling_shutter=None takes the paths the frames always came from, with and without a camera; readout 0 renders the same
    scene through the per-row path (the previous frame is then sampled bilinearly too: at most one grey level apart)."""
    import hashlib
    from of_amd import synth
    from of_amd.pipeline import CameraModel, RollingShutter
    cm = CameraModel(fx=80.0, fy=80.0, cx=40.0, cy=30.0, k=(-0.1, 0.01, 0, 0))
    for kw in ({}, dict(camera=cm)):
        a = synth.render_pair(60, 80, 3, **kw)
        b = synth.render_pair(60, 80, 3, rolling_shutter=None, **kw)
        assert np.array_equal(a["prev"], b["prev"]) and np.array_equal(a["next"], b["next"]) and "rolling_shutter" not in a
        z = synth.render_pair(60, 80, 3, rolling_shutter=RollingShutter(readout=0.0), **kw)
        assert np.abs(z["next"].astype(int) - a["next"].astype(int)).max() <= 1 and np.abs(z["prev"].astype(int) - a["prev"].astype(int)).max() <= 1
        r = synth.render_pair(60, 80, 3, rolling_shutter=RollingShutter(readout=0.9), omega=(0.002, -0.001, 0.05), **kw)
        s = synth.render_pair(60, 80, 3, omega=(0.002, -0.001, 0.05), **kw)
        assert np.abs(r["next"].astype(int) - s["next"].astype(int)).max() > 8 and np.array_equal(r["H"], s["H"])
        f0, _ = synth.render_sequence(60, 80, 3, 3, **kw)
        f1, _ = synth.render_sequence(60, 80, 3, 3, rolling_shutter=None, **kw)
        f2, _ = synth.render_sequence(60, 80, 3, 3, rolling_shutter=RollingShutter(readout=0.0), **kw)
        assert np.array_equal(f0, f1) and np.abs(f2.astype(int) - f0.astype(int)).max() <= 1
    # the bytes of today's frames, pinned: sha1 of prev + next for seed 3 at 60 x 80, without and with the camera above
    got = [hashlib.sha1(p["prev"].tobytes() + p["next"].tobytes()).hexdigest() for p in (synth.render_pair(60, 80, 3), synth.render_pair(60, 80, 3, camera=cm))]
    assert got == PINNED, got


PINNED = ["874c0b270f5f93f2ec40d912c5379f192f710a6c", "f9c445d1c95cd66ba7dd7792568c3f8cfe088e00"]
