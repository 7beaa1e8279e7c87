"""The numpy restatement of the perspective warp (tests/stabilise_reference.py) on the CPU: what the rule does at its corners, and what
the warp is for - the rendered finite-motion sequences warped into their first frame's view with the true homographies.

Measured (240 x 320, seed 5, 12 frames; gray levels 0..255; stabilised over the covered pixels / raw over the frame / cover, k = 1, 5, 11):
  v (0.004, -0.003, 0.002), omega (0.003, -0.002, 0.01):  1.82 / 1.80 / 1.82   18.9 / 34.6 / 35.9   0.988 / 0.953 / 0.903
  v (0.002,  0.001, 0),     omega (0.001,  0.002, 0.03):  1.78 / 1.78 / 1.75   25.1 / 35.3 / 35.6   0.980 / 0.924 / 0.860
The residue of about 1.8 is the bilinear blur of the texture.  The smallest gain is 10.4 (18.88 / 1.82); asserted at half of it.
Then the view's rules (pose()), the re-base by cover on the second sequence, and the CPU chain (chain()): its gain is measured in
test_cpu_chain_holds_the_ground_still's docstring."""
import numpy as np
import pytest

import stabilise_reference as sr

TABLE = (((1.82, 18.9, 0.988), (1.80, 34.6, 0.953), (1.82, 35.9, 0.903)),
         ((1.78, 25.1, 0.980), (1.78, 35.3, 0.924), (1.75, 35.6, 0.860)))


def image(h, w, ch, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, ch) if ch == 3 else (h, w), dtype=np.uint8)


@pytest.mark.parametrize("h,w", ((1, 1), (3, 5), (67, 33), (240, 320)))
@pytest.mark.parametrize("ch", (1, 3))
def test_identity_returns_the_source_and_covers_all_but_the_last_row_and_column(h, w, ch):
    src = image(h, w, ch, 1)
    for border in (sr.BORDER_CONSTANT, sr.BORDER_REPLICATE):
        out, mask = sr.warp_mask(src, np.eye(3), None, border, 200)
        assert np.array_equal(out, src)
        want = np.zeros((h, w), bool)
        want[:h - 1, :w - 1] = True
        assert np.array_equal(mask, want)


def test_whole_shift_moves_pixels_and_the_border_fills_the_rest():
    src = image(20, 30, 1, 2)
    M = np.array([[1.0, 0, 3.0], [0, 1.0, -2.0], [0, 0, 1.0]])      # destination (x, y) reads source (x + 3, y - 2)
    out, cov = sr.warp(src, M, None, sr.BORDER_CONSTANT, 200)
    assert np.array_equal(out[2:, :27], src[:18, 3:]) and np.all(out[:2] == 200) and np.all(out[:, 27:] == 200)
    assert cov == 18 * 26                                           # source columns 3..28 and rows 0..17: all four taps inside
    rep, cov2 = sr.warp(src, M, None, sr.BORDER_REPLICATE, 200)
    assert cov2 == cov and np.array_equal(rep[2:, :27], src[:18, 3:])
    assert np.array_equal(rep[0, :27], src[0, 3:]) and np.all(rep[5, 27:] == src[3, 29])


def test_half_pixel_is_the_rounded_mean_and_a_64th_is_a_tie_to_even():
    src = image(9, 9, 1, 3).astype(np.int64)
    half = np.array([[1.0, 0, 0.5], [0, 1.0, 0.5], [0, 0, 1.0]])
    out, _ = sr.warp(src.astype(np.uint8), half, (8, 8))
    want = (256 * (src[:-1, :-1] + src[:-1, 1:] + src[1:, :-1] + src[1:, 1:]) + 512) >> 10
    assert np.array_equal(out, want)
    tie = np.array([[1.0, 0, 1.0 / 64], [0, 1.0, 1.0 / 64], [0, 0, 1.0]])      # fx = 32 x + 1/2: rint goes to the even 32 x, so nothing moves
    out, _ = sr.warp(src.astype(np.uint8), tie, (8, 8))
    assert np.array_equal(out, src[:8, :8])
    tie3 = np.array([[1.0, 0, 3.0 / 64], [0, 1.0, 0.0], [0, 0, 1.0]])          # fx = 32 x + 3/2 -> 32 x + 2: a = 2
    out, _ = sr.warp(src.astype(np.uint8), tie3, (8, 8))
    assert np.array_equal(out, (32 * (30 * src[:8, :8] + 2 * src[:8, 1:9]) + 512) >> 10)


def test_pixels_that_are_not_ok_take_the_border_value_under_either_border():
    src = image(12, 16, 3, 4)
    mats = sr.matrices(12, 16, 12, 16)
    for border in (sr.BORDER_CONSTANT, sr.BORDER_REPLICATE):
        for name in ("nan", "inf", "nan_in_w"):
            out, cov = sr.warp(src, mats[name], None, border, 200)
            assert np.all(out == 200) and cov == 0, name
        out, cov = sr.warp(src, mats["limit_pos"], None, border, 200)       # columns 0..2: |fx| <= 2^30, far outside; 3..: not ok
        assert np.all(out[:, 3:] == 200) and cov == 0
        assert np.all(out[:, :3] == (200 if border == sr.BORDER_CONSTANT else src[:, 15:16]))
        out, cov = sr.warp(src, mats["limit_neg"], None, border, 200)       # columns 0, 1: not ok; 2..: ok, far to the left
        assert np.all(out[:, :2] == 200) and np.all(out[:, 2:] == (200 if border == sr.BORDER_CONSTANT else src[:, 0:1]))
        out, cov = sr.warp(src, mats["zero"], None, border, 200)            # W = 0: iw = 0, every pixel reads source (0, 0)
        assert np.all(out == src[0, 0]) and cov == 12 * 16
    out, cov = sr.warp(src, mats["perspective"], None, sr.BORDER_CONSTANT, 0)   # W < 0 right of x = 9: no sign test, the pixels map like any other
    assert 0 < cov < 12 * 16


@pytest.mark.parametrize("which", (0, 1))
def test_true_homographies_reproduce_the_measured_table_and_its_gain(pkg, which):
    gray, H = sr.sequence(which)
    rows = sr.stabilised_figures(gray, H)
    for (stab, raw, cover), k in zip(TABLE[which], (1, 5, 11)):
        s, r, c = rows[k - 1]
        print(f"sequence {which} k {k}: stabilised {s:.3f} raw {r:.3f} cover {c:.4f}")
        assert abs(s - stab) < 0.01 and abs(r - raw) < 0.1 and abs(c - cover) < 0.001
    for k, (s, r, c) in enumerate(rows, 1):
        assert s * 5.0 <= r, (k, s, r)                              # half the smallest measured gain of 10.4


def test_pose_rules_on_the_cpu():
    """The view's bookkeeping: flags, the chain across re-keys, both re-bases, the counts."""
    sn = np.zeros(28); sn[0] = 1.0; sn[3] = 1.0; sn[19] = 1.0 / 320; sn[20] = 160.0; sn[21] = 120.0
    R = np.array([[np.cos(0.02), -np.sin(0.02), 0], [np.sin(0.02), np.cos(0.02), 0], [0, 0, 1.0]])
    key = np.zeros(32); key[0:3] = (0.01, -0.02, 0.005)
    st, rec = sr.pose(R, key, sn, 240, 320)                          # solved, the plane's homography: synth's finite form
    from_synth = np.array([[320.0, 0, 160], [0, 320.0, 120], [0, 0, 1]]) @ ((np.eye(3) + np.outer(key[0:3], sn[1:4]) / (1.0 - key[2])) @ R) \
        @ np.linalg.inv(np.array([[320.0, 0, 160], [0, 320.0, 120], [0, 0, 1]]))
    assert rec[30] == sr.FULL and np.allclose(rec[0:9].reshape(3, 3), from_synth, rtol=0, atol=1e-9) and np.array_equal(st["Bv"], np.eye(3))
    assert list(st["ints"]) == [1, 0, 0, 1] and rec[36] == -1
    key[9] = 4.0                                                     # a re-key: the view is chained (chain 1) or jumps (chain 0)
    st1, rec1 = sr.pose(R, key, sn, 240, 320, st, prev_covered=70000)
    assert np.array_equal(rec1[0:9], rec[0:9]) and not np.array_equal(st1["Bv"], np.eye(3)) and rec1[34] == 0 and rec1[35] == 1
    st0, _ = sr.pose(R, key, sn, 240, 320, st, prev_covered=70000, s=sr.setting(chain=0))
    assert np.array_equal(st0["Bv"], np.eye(3))
    st2, rec2 = sr.pose(R, key, sn, 240, 320, st1, prev_covered=70000, s=sr.setting(mode=sr.STAB_ROTATION))
    assert rec2[30] == sr.ROTATION_ONLY and rec2[34] == 1            # a re-key without the translation: approx
    none = np.zeros(32); none[3] = 2.0; none[9] = 1.0
    st3, rec3 = sr.pose(R, none, sn, 240, 320, st1, prev_covered=70000)
    assert rec3[30] == sr.NONE and rec3[34] == 1 and np.allclose(rec3[0:9].reshape(3, 3), sr.pixels(st1["Bv"], sn[19], sn[20], sn[21]))
    key[9] = 0.0
    st4, rec4 = sr.pose(R, key, sn, 240, 320, st1, prev_covered=int(0.5 * 76800) - 1)        # below min_cover h w: re-based on the keyframe
    assert rec4[31] == sr.RB_COVER and np.array_equal(rec4[0:9], rec[0:9]) and list(st4["ints"]) == [0, 1, 0, 1]
    _, rec5 = sr.pose(R, key, sn, 240, 320, st1, prev_covered=int(0.5 * 76800))
    assert rec5[31] == 0 and rec5[32] == 3
    bad = dict(Bv=st1["Bv"].copy(), ints=st1["ints"]); bad["Bv"][0, 1] = np.nan
    st6, rec6 = sr.pose(R, key, sn, 240, 320, bad, prev_covered=70000)
    assert rec6[31] == sr.RB_FINITE and np.array_equal(rec6[0:9], rec[0:9]) and np.array_equal(st6["Bv"], np.eye(3))
    unsolved = key.copy(); unsolved[3] = 1.0
    assert sr.pose(R, unsolved, sn, 240, 320)[1][30] == sr.ROTATION_ONLY
    thin = key.copy(); thin[0:3] = (0.0, 0.0, 1.0)                   # the plane through the camera: d - n.T = 0
    assert sr.pose(R, thin, sn, 240, 320)[1][30] == sr.ROTATION_ONLY


def test_min_cover_rebases_the_second_sequence_between_step_5_and_step_11(pkg):
    gray, H = sr.sequence(1)
    run = sr.view_run(gray, H, 240, 320, sr.setting(min_cover=0.9))
    cover = [c / 76800.0 for _, _, c in run]
    rebases = [int(r[33]) for r, _, _ in run]
    print("cover", ["%.3f" % c for c in cover], "re-bases", rebases)
    assert abs(cover[4] - 0.924) < 0.001 and abs(cover[10] - 0.860) < 0.001
    assert rebases[4] == 0 and rebases[10] >= 1
    first = rebases.index(1)                                         # the step behind the first warp that covered less than 0.9 of the frame
    assert cover[first - 1] < 0.9 <= min(cover[:first - 1]) and run[first][0][31] == sr.RB_COVER


CHAIN_GAIN = 20.3


@pytest.mark.parametrize("which,max_age", ((0, 0), (1, 0), (0, 3), (1, 3)))
def test_cpu_chain_holds_the_ground_still(pkg, which, max_age):
    """The two sequences through the CPU chain: the C oracle's LK, the template and keyframe restatements, pose() and warp().  The view
    is frame 1's (the first step keys on it), so the figures are taken against frame 1 from frame 2 on.  Measured, smallest raw /
    stabilised mean abs diff over frames 2..11: 20.3 and 26.6 with one keyframe, 20.3 and 24.5 with max_age = 3 (three keyframes, the
    view chained across them); the stabilised diff is 0.91 .. 1.44 gray levels against a raw 18.5 .. 35.6.  Asserted at half of 20.3."""
    import keyframe_reference as K
    c = sr.chain(which, key=K.setting(max_age=max_age))
    print("sequence", which, "max_age", max_age, "gain %.2f" % c["gain"], "keyframes", c["keyframes"], ["%.2f / %.1f / %.3f" % r for r in c["rows"]])
    assert c["flags"][0] == sr.NONE and all(f == sr.FULL for f in c["flags"][1:]) and c["rebases"] == 0 and c["approx"] == 1
    assert c["keyframes"] == (3 if max_age else 1)
    assert c["gain"] >= CHAIN_GAIN / 2.0
