"""CPU-only: the corner-grid entry points exist in the header, the binding and the library; the struct and the cell limit agree on
both sides; the grid kernel is in the code object."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofk_set_corner_grid", "ofk_get_corner_grid", "ofk_corner_grid_download", "ofk_select_corners_grid", "ofk_good_features_grid")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge


def test_entry_points_declared_bound_and_exported(built, ofk):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofk.h")).read(), flags=re.S)
    lib = ofk.load_library()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert s in ofk.SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
    m = re.search(r"#define\s+OFK_GRID_MAX_CELLS\s+(\d+)", txt)
    assert m and int(m.group(1)) == ofk.GRID_MAX_CELLS == 2048
    m = re.search(r"typedef struct ofk_corner_grid \{(.*?)\} ofk_corner_grid;", txt, flags=re.S)
    assert m and re.findall(r"\b(int|double)\s+(\w+);", m.group(1)) == [("int", "cell"), ("int", "cap"), ("int", "max_rank")]
    assert [(n, t) for n, t in ofk.CornerGrid._fields_] == [("cell", C.c_int), ("cap", C.c_int), ("max_rank", C.c_int)]
    assert len(lib.ofk_good_features_grid.argtypes) == len(lib.ofk_good_features.argtypes) + 4
    assert len(lib.ofk_select_corners_grid.argtypes) == len(lib.ofk_select_corners.argtypes) + 4


def test_grid_kernel_is_in_the_code_object(built, ofk):
    blob = open(ofk.LIB_PATH, "rb").read()
    assert b"k_select_greedy_grid" in blob
