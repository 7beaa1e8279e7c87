"""CPU-only: libofk.so builds for gfx950, loads through ctypes and exports every symbol include/ofk.h declares;
the product never imports or links the oracle; without a GPU the entry points fail loudly (no CPU fallback)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "drone-stabilisation-using-optical-flow-gps-and-inertial-sensors_amd")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "ofk.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(ofk_[a-z0-9_]+)\s*\(", txt)))


def test_header_and_binding_agree(built, ofk):
    assert header_symbols() == sorted(ofk.SYMBOLS)


def test_library_exports_every_declared_symbol(built, ofk):
    lib = ofk.load_library()
    for s in header_symbols():
        assert hasattr(lib, s), s
    assert lib.ofk_version() == 100
    out = subprocess.check_output(["nm", "-D", "--defined-only", ofk.LIB_PATH], text=True)
    exported = set(re.findall(r" T (ofk_\w+)", out))
    assert set(header_symbols()) <= exported


def test_code_object_is_gfx950_only(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    for other in (b"gfx90a", b"gfx942", b"sm_80", b"nvptx"):
        assert other not in blob


def test_product_never_touches_the_oracle():
    bad = []
    for dirpath, _, files in os.walk(PKG):
        if "build" in dirpath.split(os.sep):
            continue
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", "Makefile")) or f == "velocity_measurment_node":
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                if re.search(r"^\s*(from|import)\s+oracle\b|oracle/_build|liboracle|orc_[a-z_]+\(", txt, flags=re.M):
                    bad.append(os.path.join(dirpath, f))
    assert not bad, bad


def test_no_gpu_fails_loudly(built, ofk):
    lib = ofk.load_library()
    if lib.ofk_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(ofk.OfkError):
        ofk.Context(0, 640, 480, 1, 64, 3)


def test_jpeg_pass_counter_is_declared_bound_and_null_safe(built, ofk):
    """ofk_jpeg_last_iterations: in the header, in the binding, exported; a read-only query that answers 0 where no decode has run -
    a NULL context included (no GPU needed for that)."""
    assert "ofk_jpeg_last_iterations" in header_symbols() and "ofk_jpeg_last_iterations" in ofk.SYMBOLS
    lib = ofk.load_library()
    assert lib.ofk_jpeg_last_iterations(None) == 0
    assert callable(ofk.Context.jpeg_last_iterations)
