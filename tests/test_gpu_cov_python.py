"""GPU: the Python layers over the velocity covariance - velocity_node.solve_lgs_cov, simulation.predict_sweep and
optical_fusion(cov=...), which fills the vel_err attribute the reference carries and never reads - against tests/cov_reference.py."""
import os
import types

import numpy as np
import pytest

import cov_reference as cr
from oracle import estimation_oracle as eo

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_solve_lgs_cov(pkg, ofk):
    from of_amd.velocity_node import solve_lgs_cov, solve_lgs
    rng = np.random.default_rng(4)
    x = rng.uniform(-0.7, 0.7, (40, 2)); nrm = np.array([0.03, -0.05, 1.0]); nrm /= np.linalg.norm(nrm)
    om = np.array([0.1, -0.2, 0.15]); d = 1.7
    u = eo.generate_test_data(x, [0.4, -0.3, 0.2], om, d, nrm) + rng.normal(0, 1e-3, (40, 2))
    sig = dict(sigma_flow=0.002, sigma_pos=0.003, sigma_d=0.04, sigma_omega=(0.01, 0.02, 0.015), sigma_normal=0.004)
    v, R, rank, s, Cv, rec = solve_lgs_cov(x, u, d, nrm, om, **sig)
    v0, R0, rank0, s0 = solve_lgs(x, u, d, nrm, om)
    assert np.array_equal(v, v0) and np.array_equal(R, R0) and rank == rank0 == 3 and np.array_equal(s, s0)
    ref = cr.covariance(cr.NODE, x, u, d, nrm, om, cr.sigmas(**sig), v=v, rss=R[0], rank=3)
    assert np.abs(Cv - cr.untri(ref[0:6])).max() <= 1e-9 * np.abs(ref[0:6]).max() and np.array_equal(Cv, Cv.T)
    assert np.abs(rec[16:22] - ref[16:22]).max() <= 1e-9 * ref[16:22].max()
    v, R, rank, s, Cv, rec = solve_lgs_cov(x, u, d, nrm, om, mode="residual")
    ref = cr.covariance(cr.NODE, x, u, d, nrm, om, cr.sigmas(), cr.RESIDUAL, v=v, rss=R[0], rank=3)
    assert np.abs(Cv - cr.untri(ref[0:6])).max() <= 1e-9 * np.abs(ref[0:6]).max()
    v, R, rank, s, Cv, rec = solve_lgs_cov(x[:1], u[:1], d, nrm, om, **sig)
    assert rank < 3 and not Cv.any() and rec[13] == 1


def test_predict_sweep_is_the_reference_prediction(pkg, ofk):
    import of_amd.simulation as sim
    raw = np.load(os.path.join(HERE, "golden", "reference_sweeps.npz"))["points_raw"]
    truth = ([1.0, 1, 1], [1.0, 1, 1], 1.0, [0.0, 0, 1], [0.02, 0, 0.205])
    for axis, steps in (("flow_errors", (10, 50)), ("ang_vel_error", (90,)), ("translation_error", (30,)), ("distance_error", (70,))):
        got = sim.predict_sweep(axis, raw, *truth, steps=steps)
        assert got.shape == (len(steps), 3)
        for row, i in enumerate(steps):
            x, h, n, sg = sim.sweep_step(axis, i, 100, raw, truth[2], truth[3], None)
            u = eo.generate_test_data(x, truth[0], truth[1], h, n, truth[4])
            ref = cr.predict_std(cr.SIM, x, u, h, n, np.array(truth[1]), cr.sigmas(sigma_omega=sg[0], sigma_offset=sg[1], sigma_d=sg[2], sigma_flow=sg[3],
                                                                                 sigma_pos=sg[4]), t=np.array(truth[4]))
            np.testing.assert_allclose(got[row], ref, rtol=1e-8)
    assert sim.predict_sweep("flow_errors", raw, *truth, k=4).shape == (4, 3)


def test_optical_fusion_fills_vel_err(pkg, ofk):
    from of_amd import synth
    from of_amd import velocity_node as node
    cov = dict(mode="propagate", sigma_flow_px=0.3, sigma_pos_px=0.5, sigma_d=0.05, sigma_omega=0.01, sigma_offset=0.005)
    # the node as shipped: four test features, the solve on the host's points
    n = node.optical_fusion(spin=False, cov=cov)
    frame = np.zeros((48, 64, 3), np.uint8)
    n.call_optical(frame); n.call_optical(frame)
    n.ang = np.array([0.01, -0.02, 0.015]); n.rotation = eo.quat_to_rot(0.1, -0.05, 0.2, np.sqrt(1 - 0.0525)); n.normal = np.array([0, 0, 1.0])
    assert list(n.vel_err) == [0.1, 0.1, 0.1]
    assert n.step() is not None and n.last_cov is not None and n.last_cov[13] == 0
    R = np.asarray(n.rotation)
    want = np.sqrt(np.diag(R @ ofk.cov_matrix(n.last_cov[6:12]) @ R.T))
    assert np.array_equal(n.vel_err, want) and np.all(n.vel_err > 0) and np.all(np.isfinite(n.vel_err))
    plain = node.optical_fusion(spin=False)
    plain.call_optical(frame); plain.call_optical(frame)
    plain.ang = n.ang; plain.rotation = n.rotation; plain.normal = n.normal
    assert plain.step() is not None and list(plain.vel_err) == [0.1, 0.1, 0.1] and plain.last_cov is None
    # the restored pipeline: the record of the resident stream step
    p = synth.render_pair(480, 640, 31, v=(0.01, -0.008, 0.004), omega=(0, 0, 0), d=0.75, scaling=0.01)
    outs = []
    for kw in ({}, dict(cov=cov)):
        m = node.optical_fusion(spin=False, synthetic_test=False, **kw)
        m.feature_params = dict(qualityLevel=0.05, minDistance=10, blockSize=12)
        m.T = 2.0
        m.call_optical(p["prev"]); m.call_optical(p["next"])
        outs.append((m, m.step()))
    (a, va), (b, vb) = outs
    assert va is not None and np.array_equal(va, vb) and list(a.vel_err) == [0.1, 0.1, 0.1]
    rec = b._stream.covariances()[0]
    assert rec[13] == 0 and np.array_equal(b.vel_err, np.sqrt(rec[[6, 9, 11]])) and np.all(b.vel_err > 0)
    assert np.array_equal(rec, b.last_cov)
