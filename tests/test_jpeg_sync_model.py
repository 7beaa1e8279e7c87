"""CPU-only: the synchronisation model (tests/jpeg_sync_model.py) that chooses the inputs of tests/test_gpu_jpeg_edges.py.

The model's fixed point must be the serial decode (else its pass counts mean nothing), a textured frame must be the quick case
the decoder was built for, and every stream tests/golden/jpeg_edges.npz labels slow must be as slow as the GPU test that uses it
needs: these are conditions on the INPUTS - the device is not held to the model's counts (a device pass may be ahead of the Jacobi
schedule)."""
import os

import numpy as np
import pytest

import jpeg_sync_model as model
from jpeg_edges_cases import Edges
from oracle import jpeg_oracle as jo

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_golden.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def edges():
    return Edges()


@pytest.fixture(scope="module")
def slow(edges):
    """(chunks, passes) at 64-byte chunks of every fixture that carries a condition: modelled once for the module"""
    return {n: model.passes(edges.jpg(n), 64) for n in edges.conditions}


def _streams(gold, edges):
    for n in ("c420_ros", "c420_odd", "c420_q100", "c420_q20", "c422", "c444", "gray"):
        yield n, gold[f"jpg_{n}"].tobytes()
    for n in ("stripes_72x320", "black_480x640_420", "opt_444_240x320", "opt_gray_240x320", "tex_72x320_a", "tiny_1x1_420_noise", "tiny_3x3_422_noise",
              "tiny_24x40_420_noise", "tiny_15x17_gray_noise2"):
        yield n, edges.jpg(n)


def test_fixed_point_is_the_serial_decode(pkg, ofk, gold, edges):
    """Entry state and completed blocks of every chunk at the fixed point = those of ONE decoder that walks the stream from its
    true start; that decoder completes the frame's last block (the oracle's block count) in the stream's last byte; the model reads
    the entropy bytes the host stages (ofk_jpeg_destuff)."""
    for name, data in _streams(gold, edges):
        scan = model.parse(data)
        assert scan.ent == ofk.jpeg_destuff(data)[0], name
        assert scan.nblk == jo.info(data)["nblocks"], name
        for jch in (64, 256):
            entry, counts, end = model.serial(scan, jch)
            r = model.iterate(scan, jch, max_passes=len(entry) + 2)
            assert r["chunks"] == len(entry) == len(scan.ent) // jch + 1
            assert r["entry"] == entry and r["counts"] == counts, (name, jch)
            assert end is not None and (end + 7) // 8 == len(scan.ent), (name, jch, end, len(scan.ent))
            assert sum(counts) >= scan.nblk and sum(counts[:-1]) < scan.nblk, (name, jch)      # (the last chunk runs on into the zero padding)
            assert r["passes"] <= r["chunks"] + 1                  # the truth advances at least one chunk per pass


def test_model_refuses_restart_intervals(gold):
    with pytest.raises(ValueError, match="restart"):
        model.parse(gold["jpg_c420_rst_rows"].tobytes())


def test_textured_frame_synchronises_quickly(gold, edges):
    chunks, passes = model.passes(gold["jpg_c420_ros"].tobytes(), 64)
    assert chunks > 100 and passes < 16, (chunks, passes)
    for n in ("tex_72x320_a", "tex_72x320_b"):                  # the textured members of the mixed batches
        chunks, passes = model.passes(edges.jpg(n), 64)
        assert chunks > 50 and passes < 16, (n, chunks, passes)


def test_slow_fixtures_are_as_slow_as_their_tests_need(edges, slow):
    """The pass-count condition each slow fixture was generated for, at 64-byte chunks: one stripes stream per look window of the host
    loop around the end of its 64 flag slots (passes 56-59, 60-63, 64-67, 68-71), 72x320 among them; two stripes streams and the
    1080p flat frame at 128 passes or more; the 480x640 flat frames behind slot 63.  Slow here means what the header of k_jpeg.hip
    names as the worst case: about one pass per chunk."""
    cond = edges.conditions
    assert sorted((lo, hi) for n, (lo, hi) in cond.items() if hi < 1000) == [(56, 59), (60, 63), (64, 67), (68, 71)]
    assert cond["stripes_72x320"] == (64, 67)
    assert sum(lo >= 128 for n, (lo, hi) in cond.items() if n.startswith("stripes")) >= 2 and cond["black_1080x1920_420"][0] >= 128
    assert cond["black_480x640_420"][0] >= 64 and cond["white_480x640_420"][0] >= 64
    for name, (lo, hi) in cond.items():
        chunks, passes = slow[name]
        assert lo <= passes <= hi, (name, chunks, passes, lo, hi)
        assert passes >= chunks - 2, (name, chunks, passes)
    assert slow["stripes_72x320"] == (66, 65)


def test_fitted_tables_of_flat_frames_give_an_all_zero_bit_stream(edges):
    """optimize=True on a flat frame: one-bit codes for the only DC and AC symbols; every bit of the entropy segment but the padding of
    its last byte is zero - the other end of the scale from white noise for the first-level table."""
    for n in ("opt_gray_240x320", "opt_444_240x320", "opt_420_240x320"):
        scan = model.parse(edges.jpg(n))
        assert len(scan.ent) > 64 and not any(scan.ent[:-1]), n
        for dc, ac in scan.tab:
            assert dc[0] >> 8 == 1 and ac[0] >> 8 == 1, n       # a 0 bit is a complete code in both tables


def test_host_loop_needs_the_reused_slot_cleared(edges, slow):
    """A CPU copy of jdecode_staged's loop (model.host_loop) over the modelled pass counts: the four window streams end at the look
    their window names, the >= 128-pass streams end with more than 64 passes queued - and WITHOUT the memset in front of every pass
    that reuses the last flag slot the loop never sees a clear flag again once pass 63 has set it: it runs into the non-convergence
    guard.  That is what the GPU tests of those streams would report if the slot handling broke."""
    looks = {}
    for name, (lo, hi) in edges.conditions.items():
        chunks, passes = slow[name]
        queued, how = model.host_loop(passes, chunks)
        assert how == "converged" and passes <= queued <= passes + 3, (name, passes, queued)
        looks[name] = queued
        queued2, how2 = model.host_loop(passes, chunks, clear_reused_slot=False)
        if passes <= 63:
            assert (queued2, how2) == (queued, how), name
        else:
            assert how2 == "guard" and queued2 > chunks + 2, (name, queued2, how2)
    assert sorted(q for n, q in looks.items() if edges.conditions[n][1] < 1000) == [59, 63, 67, 71]
    assert looks["stripes_160x320"] > 64 and looks["stripes_240x320"] > 64
    assert model.host_loop(1, 1) == (0, "converged")             # single-chunk batch: no pass behind the first
    assert model.host_loop(1, 2) == (7, "converged")             # quiet from pass 1 on: the first burst is all that goes out
