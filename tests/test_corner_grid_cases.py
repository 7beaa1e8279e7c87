"""CPU companion of tests/test_gpu_corner_grid.py: on the reference alone, no case of tests/corner_grid_cases.py is vacuous - the
binding ones differ from the plain selection, the deep ones walk past the 512 keys of the first cut, the full ones end with every cell
full and budget left, the in-round ones meet more than `cap` candidates of one cell inside one aligned run of 64."""
import numpy as np
import pytest

import corner_grid_cases as K
import corner_grid_reference as R


def _cells(case):
    h, w = K.scene(case["scene"]).shape
    cell = case["grid"][0]
    return -(-w // cell) * -(-h // cell)


@pytest.mark.parametrize("case", K.CASES, ids=[c["id"] for c in K.CASES])
def test_case_is_not_vacuous(case):
    ref, plain = K.reference(case), K.reference(case, plain=True)
    want = set(case["designated"])
    assert want and _cells(case) <= R.MAX_CELLS
    differs = [not np.array_equal(r[0], p[0]) for r, p in zip(ref, plain)]
    if "binds" in want:
        assert all(differs)
    if "plain" in want:
        assert not any(differs) and all(r[1][0] > 0 for r in ref)
    if "deep" in want:
        assert all(r[1][1] > 512 for r in ref)
    if "full" in want:
        cell, cap, _ = case["grid"]
        h, w = K.scene(case["scene"]).shape
        for pts, (acc, _), _ in ref:
            occ = R.occupancy(h, w, cell, pts)
            assert (occ >= cap).all() and acc < case["max_corners"] and acc == _cells(case) * cap
    if "inround" in want:
        e = K.eig_of(case["scene"], case["block"])
        h, w = e.shape
        cell, cap, _ = case["grid"]
        idx = R.candidates(e, case["quality"])[:ref[0][1][1]]
        cells = (idx // w // cell) * -(-w // cell) + (idx % w) // cell
        assert max(np.bincount(cells[i:i + 64]).max() for i in range(0, len(idx), 64)) > cap


def test_the_list_covers_what_it_must():
    by = {c["id"]: c for c in K.CASES}
    assert _cells(by["a-one-cell"]) == 1
    assert _cells(by["tiny-cell1"]) == R.MAX_CELLS and K.scene("tiny").shape == (32, 64)
    occ = by["a-occupancy"]
    counts = occ["occ"][1]
    assert len(set(counts.tolist())) == 3 and 0 in counts        # a ragged batch, one image without a list
    accepted = [r[1][0] for r in K.reference(occ)]
    assert accepted[1] == 0 and accepted[0] > 0 and accepted[2] > 0                  # every cell closed / some / none
    assert not np.array_equal(K.reference(occ)[0][0], K.reference(occ)[2][0])        # the partial list changes the answer
    ranks = sorted(c["grid"][2] for c in K.CASES if c["grid"][2])
    assert ranks[0] < 512 and 512 in ranks and any(512 < r < 565 for r in ranks)     # below, at and beyond the first 512 keys
    assert by["a-mask"]["mask"] is not None
    big = by["big-1200"]
    assert big["max_corners"] >= 1024 and K.reference(big)[0][1][0] < big["max_corners"]
    for c in K.PLATEAU_CASES:
        ref, plain = K.plateau_reference(c), K.plateau_reference(c, plain=True)
        assert not np.array_equal(ref[0], plain[0]) and ref[1][0] > 0
    vals = np.unique(K.plateau_map())
    assert len(vals) == 4 and len(R.candidates(K.plateau_map(), 0.01)) > 1024       # heavy ties: the first histogram bin overflows
