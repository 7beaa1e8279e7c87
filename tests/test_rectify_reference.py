"""The warp through a lens on the CPU (ofk.h: ofk_warp_lens; tests/rectify_reference.py): the restatement against the plain warp's, what
rectification buys on the rendered sequences, r_max, CameraModel.ideal_radius, and the condition that makes the GPU test's fisheye
comparison exact (no coordinate within FISH_TIE of a rounding tie).  No GPU."""
import numpy as np
import pytest

import camera_reference as cr
import rectify_reference as rr
import stabilise_reference as sr


def image(h, w, ch, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, ch) if ch == 3 else (h, w), dtype=np.uint8)


@pytest.mark.parametrize("ch", (1, 3))
@pytest.mark.parametrize("border,bval", ((sr.BORDER_CONSTANT, 7), (sr.BORDER_REPLICATE, 200)))
def test_without_a_lens_it_is_the_plain_warp_bit_for_bit(ch, border, bval):
    """All coefficients zero, unit camera and output matrices: Mn = M, xd = xn, and X (1 / W) 32 = X (32 / W) in binary floating point.
    With a camera matrix Ko on the output side, M and Ko Mn describe the same map: powers of two keep every quotient exact."""
    unit = cr.camera(cr.BROWN, (), 1.0, 1.0, 0.0, 0.0)
    two = cr.camera(cr.BROWN, (), 4.0, 4.0, 0.0, 0.0, fo_x=0.5, fo_y=0.5)      # raw = 8 x ideal pixels
    for ssize, dsize in (((67, 33), (64, 16)), ((5, 257), (3, 5)), ((1, 1), (1, 1))):
        src = image(*ssize, ch, 3)
        for name, M in sr.matrices(*ssize, *dsize).items():
            want, wmask = sr.warp_mask(src, M, dsize, border, bval)
            got, mask, _ = rr.warp_lens(src, M, unit, dsize, border, bval)
            assert np.array_equal(got, want) and np.array_equal(mask, wmask), (name, ssize, dsize)
            if np.all(np.isfinite(M)):
                got, mask, _ = rr.warp_lens(src, M / np.array([[8.0], [8.0], [1.0]]), two, dsize, border, bval)
                assert np.array_equal(got, want) and np.array_equal(mask, wmask), (name, ssize, dsize, "scaled")
    src = image(9, 11, ch, 4)
    got, mask, _ = rr.warp_lens(src, None, unit)
    assert np.array_equal(got, src) and np.count_nonzero(mask) == 8 * 10


# mean |rectified raw frame - the same scene rendered without a lens| in gray levels, measured here: both are bilinear samples of one
# texture, the rectified one sampled twice.  MILD 1.56, STRONG 1.93, FISH 1.98 (largest single pixel: 16); asserted at twice that.
RECTIFY_DEV = dict(MILD=1.56, STRONG=1.93, FISH=1.98)


@pytest.mark.parametrize("lens", ("MILD", "STRONG", "FISH"))
def test_rectifying_a_lens_rendered_frame_gives_the_scene_without_the_lens(pkg, lens):
    raw, plain, _, cam, _, _ = rr.lens_sequence(0, lens)
    out, mask, _ = rr.warp_lens(raw[0], None, cam)
    dev = float(np.abs(out.astype(np.int32) - plain[0].astype(np.int32))[mask].mean())
    unrect = float(np.abs(raw[0].astype(np.int32) - plain[0].astype(np.int32)).mean())
    print(lens, "rectified against the lens-free scene", dev, "raw against it", unrect, "cover", mask.mean())
    assert mask.mean() >= 0.98
    assert dev <= 2.0 * RECTIFY_DEV[lens], dev
    assert lens == "MILD" or unrect >= 4.0 * dev                   # the strong lenses move the picture by many pixels


# per lens and motion, measured here (frames 1-11 against frame 0 rectified, true homographies in ideal pixels, gray levels over the
# covered pixels): lens warp | plain k_warp_u8 rule on the raw frame against raw frame 0 | raw frames | smallest raw / lens warp
#   MILD   0  0.94-0.97 | 1.15- 2.90 | 16.02-34.80 | 16.8        MILD   1  0.90-0.95 | 1.18- 3.40 | 24.49-35.44 | 25.7
#   STRONG 0  0.99-1.02 | 2.57-15.94 | 16.36-34.89 | 16.0        STRONG 1  0.94-1.00 | 2.32-13.57 | 25.36-35.31 | 25.9
#   FISH   0  1.00-1.05 | 3.09-18.46 | 16.49-34.88 | 15.7        FISH   1  0.95-1.01 | 2.78-15.83 | 25.49-35.33 | 25.6
# cover 0.88-1.00.  The gain is asserted at half the smallest figure.
TABLE_GAIN = 15.7


def table_rows(which, lens):
    raw, _, H, cam, _, _ = rr.lens_sequence(which, lens)
    ref = rr.warp_lens(raw[0], None, cam)[0].astype(np.int32)
    rows, tie = [], np.inf
    for k in range(1, len(raw)):
        out, mask, t = rr.warp_lens(raw[k], H[k], cam)
        lens_d = float(np.abs(out.astype(np.int32) - ref)[mask].mean())
        pw, pm = sr.warp_mask(raw[k], H[k])
        plain_d = float(np.abs(pw.astype(np.int32) - raw[0].astype(np.int32))[pm].mean())
        raw_d = float(np.abs(raw[k].astype(np.int32) - raw[0].astype(np.int32)).mean())
        rows.append((lens_d, plain_d, raw_d, float(mask.mean())))
        tie = min(tie, float(t.min()))
    return rows, tie


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("lens", ("MILD", "STRONG", "FISH"))
def test_true_homographies_hold_the_ground_still_behind_a_lens(pkg, which, lens):
    rows, tie = table_rows(which, lens)
    a = np.array(rows)
    print(lens, which, "lens %.2f-%.2f plain %.2f-%.2f raw %.2f-%.2f cover %.2f-%.2f smallest tie distance %.3g"
          % (a[:, 0].min(), a[:, 0].max(), a[:, 1].min(), a[:, 1].max(), a[:, 2].min(), a[:, 2].max(), a[:, 3].min(), a[:, 3].max(), tie))
    assert (a[:, 2] / a[:, 0]).min() >= TABLE_GAIN / 2.0
    assert a[:, 3].min() >= 0.8
    if lens != "MILD":                                           # lifting the refusal without the lens's map would be wrong by this much
        assert np.all(a[:, 0] < a[:, 1]) and a[:, 1].max() >= 10.0 * a[:, 0].max()
    if lens == "FISH":                                           # the device's atan deviates by ~1e-11 fixed-point units: these frames are exact there
        assert tie >= rr.FISH_TIE, tie


def test_r_max_keeps_the_fold_of_a_brown_polynomial_out_of_the_view(pkg):
    """STRONG's radial polynomial turns back beyond the field of view: ideal points far out land INSIDE the raw frame.  A view shifted
    by 500 pixels looks out there; with r_max = 1.05 x the frame's ideal radius those pixels are border and not covered."""
    from of_amd.pipeline import CameraModel
    raw, _, _, cam, _, _ = rr.lens_sequence(0, "STRONG")
    rmax = 1.05 * CameraModel(**rr.seq_camera(cr.STRONG)[1]).ideal_radius(rr.SEQ["h"], rr.SEQ["w"])
    M = np.array([[1.0, 0, 500.0], [0, 1.0, 0.0], [0, 0, 1.0]])
    free, fmask, _ = rr.warp_lens(raw[0], M, cam, None, sr.BORDER_CONSTANT, 255)
    out, mask, _ = rr.warp_lens(raw[0], M, cam, None, sr.BORDER_CONSTANT, 255, rmax)
    h, w = raw[0].shape
    x = np.arange(w)[None, :] + 500.0
    y = np.arange(h)[:, None] + 0.0
    r = np.sqrt(((x - cam["co_x"]) / cam["fo_x"]) ** 2 + ((y - cam["co_y"]) / cam["fo_y"]) ** 2)
    beyond = r > rmax * (1 + 1e-12)
    assert np.count_nonzero(fmask & beyond) > 1000               # the fold: covered pixels that no ray of the lens reaches
    assert np.all(out[beyond] == 255) and not np.any(mask[beyond])
    inside = r < rmax * (1 - 1e-12)
    assert np.array_equal(out[inside], free[inside]) and np.array_equal(mask[inside], fmask[inside])
    assert np.array_equal(rr.warp_lens(raw[0], M, cam, None, sr.BORDER_REPLICATE, 9, rmax)[0][beyond], np.full(np.count_nonzero(beyond), 9, np.uint8))


@pytest.mark.parametrize("lens", ("MILD", "STRONG", "FISH"))
def test_ideal_radius_is_the_brute_force_maximum_over_the_border(pkg, lens):
    from of_amd.pipeline import CameraModel
    for h, w in ((24, 32), (1, 7), (5, 1)):
        model, k, iters = rr.LENSES[lens]
        kw = dict(fx=25.0, fy=25.2, cx=16.3, cy=11.7)
        cam = cr.camera(model, k, **kw, iters=iters)
        cm = CameraModel(model="brown" if model == cr.BROWN else "fisheye", k=tuple(k), iters=iters, **kw)
        assert cm.ideal_radius(h, w) == rr.ideal_radius(cam, h, w), (lens, h, w)
    assert CameraModel(fx=100.0, cx=4.0, cy=3.0).ideal_radius(7, 9) == np.sqrt(0.04 ** 2 + 0.03 ** 2)      # no lens: the corner's radius
    with pytest.raises(ValueError):                                # a radius that is no number is refused here, not as an r_max later
        CameraModel(fx=1e-200, cx=4.0, cy=3.0).ideal_radius(7, 9)


def test_every_fisheye_input_of_the_gpu_test_is_free_of_rounding_ties():
    """The GPU test compares the fisheye's frames bit for bit although the device's atan is another library's: a coordinate changes its
    rounded value only within ~1e-11 fixed-point units of a tie (k + 1/2), and no input comes within FISH_TIE = 1e-8 of one."""
    smallest = np.inf
    for ssize, dsize in rr.PAIRS:
        cam, r_max = rr.cameras(*ssize)["fisheye"]
        for name, M in rr.matrices(*ssize, *dsize).items():
            fx, fy, ok = rr.coordinates(M, cam, *dsize, r_max)
            with np.errstate(all="ignore"):
                t = np.minimum(np.abs(np.abs(fx - np.floor(fx)) - 0.5), np.abs(np.abs(fy - np.floor(fy)) - 0.5))
            t = np.where(ok, t, np.inf)
            smallest = min(smallest, float(t.min()))
            assert t.min() >= rr.FISH_TIE, (ssize, dsize, name, float(t.min()))
    print("smallest distance to a tie over the GPU test's fisheye inputs", smallest)


LENS_CHAIN_GAIN = 21.4


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("lens", ("STRONG", "FISH"))
def test_cpu_chain_holds_the_ground_still_behind_a_lens(pkg, which, lens):
    """stabilise_reference.chain()'s stages with the camera on (rectify_reference.chain), max_age = 3: LK and the templates on the raw
    frames, the keyframe on the ideal pixels, the raw frames warped through the lens into the view.  Measured, smallest raw /
    stabilised mean abs diff over frames 2..11: STRONG 22.3 and 21.9, FISH 21.4 and 24.1 (stabilised 0.71 .. 1.59 gray levels): as
    still as without a lens (20.3 and 24.5).  Asserted at half of 21.4."""
    import keyframe_reference as K
    c = rr.chain(which, lens, key=K.setting(max_age=3))
    print(lens, "sequence", which, "gain %.2f" % c["gain"], "keyframes", c["keyframes"], ["%.2f / %.1f / %.3f" % r for r in c["rows"]])
    assert c["flags"][0] == sr.NONE and all(f == sr.FULL for f in c["flags"][1:]) and c["rebases"] == 0 and c["approx"] == 1
    assert c["keyframes"] == 3
    assert c["gain"] >= LENS_CHAIN_GAIN / 2.0
