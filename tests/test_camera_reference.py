"""The camera model on the CPU (tests/camera_reference.py, the numpy restatement of include/ofk.h): what an uncorrected lens costs the
velocity solve and what the model gives back, the round trip of the two maps, why the default iteration count is not cv2's 5, and a
rendered scene seen through the lens.

The distorted 480 x 640 scene (synth.render_pair, f = 500, Brown -0.28 0.09 0.0008 -0.0005 -0.012, seed 5, v = (0.02, -0.015, 0.004),
omega = (0.004, -0.003, 0.01), d = 1, 200 corners) through the C oracle chain, relative error of v:
    the same scene without a lens   0.0111
    through the lens, with the model 0.0140
    through the lens, without it     0.1405
"""
import numpy as np
import pytest

import batch_oracle as BO
import camera_reference as R

@pytest.mark.parametrize("lens", [R.MILD, R.STRONG, R.FISH], ids=["brown_mild", "brown_strong", "fisheye"])
def test_uncorrected_lens_costs_the_solve_and_the_model_gives_it_back(lens):
    r = R.experiment(lens)                                       # iters 5 / 5 / 10
    print(lens[1], r)
    assert r["today"] >= 0.01, r
    assert r["model"] <= 1e-3, r


@pytest.mark.parametrize("lens", [R.MILD, R.STRONG, R.FISH], ids=["brown_mild", "brown_strong", "fisheye"])
def test_round_trip_over_the_frame(lens):
    worst, excluded = R.round_trip(R.frame_camera(lens, iters=30))
    print(lens[1], worst, excluded)
    assert excluded == 0 and worst <= 1e-3, (worst, excluded)


def test_five_iterations_are_not_enough_on_the_strong_lens():
    worst, excluded = R.round_trip(R.frame_camera(R.STRONG, iters=5))
    print(worst)
    assert excluded == 0 and worst > 0.1, worst


def test_fallback_rule():
    cam = R.frame_camera(R.STRONG, iters=30)
    pts = np.array([[100.0, 200.0], [np.nan, 5.0], [np.inf, 7.0]], np.float32)
    out, good = R.undistort_points(cam, pts, full=True)
    assert good.tolist() == [True, False, False] and np.isnan(out[1, 0]) and np.isinf(out[2, 0])      # the linear map of the input
    # coefficient sets that blow up at (500, 0) of a camera with f = 1000, c = 0: x0 = 0.5, r2 = 0.25, and 1 + k1 r2 is 0 (a pole: the
    # result is not finite) or 2.5e-8 after one round (finite, 2e10 pixels)
    pts = np.array([[500.0, 0.0], [100.0, 50.0]], np.float32)
    for cam in (R.blow_up_camera(-4.0, 20), R.blow_up_camera(-3.9999999, 1)):
        out, good = R.undistort_points(cam, pts, full=True)
        assert good.tolist() == [False, True], good
        assert np.array_equal(out[0], pts[0])                    # the linear map with P = the camera matrix: the point itself
    out, good = R.distort_points(R.camera(R.BROWN, (0, 0, 0, 0, 0, -4.0), 1000.0, 1000.0, 0.0, 0.0), pts, full=True)
    assert good.tolist() == [False, True] and np.array_equal(out[0], pts[0])


def test_rendered_scene_through_the_lens(pkg):
    plain, lens, sr, cfg, _, cam = R.scene_frames()
    e_plain = R.rel_err(BO.oracle_chain(plain["prev"], plain["next"], cfg, sr)["v"])
    chain = BO.oracle_chain(lens["prev"], lens["next"], cfg, sr)
    e_off, e_on = R.rel_err(chain["v"]), R.rel_err(R.solve_ideal(cam, chain, sr)[0])
    print("no lens", e_plain, "with the model", e_on, "without it", e_off)
    assert e_on <= 2.0 * e_plain, (e_on, e_plain)
    assert e_off >= 5.0 * e_plain, (e_off, e_plain)


def test_synth_without_a_camera_is_what_it_was(pkg):
    """camera=None takes the path the benchmark's frames come from; the camera path renders the previous frame through the lens too."""
    from of_amd import synth
    from of_amd.pipeline import CameraModel
    a = synth.render_pair(60, 80, 3)
    b = synth.render_pair(60, 80, 3, camera=None)
    assert np.array_equal(a["prev"], b["prev"]) and np.array_equal(a["next"], b["next"]) and "camera" not in a
    ident = CameraModel(fx=80.0, fy=80.0, cx=40.0, cy=30.0, k=(0, 0, 0, 0))       # no lens term: the ideal grid is the pixel grid
    xx, yy = synth.ideal_grid(60, 80, ident)
    gy, gx = np.mgrid[0:60, 0:80]
    assert np.allclose(xx, gx, atol=1e-9) and np.allclose(yy, gy, atol=1e-9)
    c = synth.render_pair(60, 80, 3, scaling=1 / 80.0)
    d = synth.render_pair(60, 80, 3, camera=ident)
    assert np.abs(c["prev"].astype(int) - d["prev"].astype(int)).max() <= 1 and np.abs(c["next"].astype(int) - d["next"].astype(int)).max() <= 1
    f, info = synth.render_sequence(60, 80, 3, 2, camera=CameraModel(fx=80.0, fy=80.0, cx=40.0, cy=30.0, k=(-0.1, 0.01, 0, 0)))
    assert f.shape == (2, 60, 80, 3) and info["scaling"] == 1 / 80.0
