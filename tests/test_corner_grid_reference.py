"""CPU-only: the numpy restatement of the capped selection (tests/corner_grid_reference.py).  With the cap off it is the oracle's
goodFeaturesToTrack selection; hand-made maps pin ties, the cap, occupancy and max_rank; the configuration's defaults mean off; and,
on the reference alone, the grid takes the corners off a high-contrast object the plain selection spends its budget on."""
import numpy as np
import pytest

from oracle import image_oracle as io
import corner_grid_cases as K
import corner_grid_reference as R


@pytest.mark.parametrize("h,w", [(480, 640), (240, 320), (243, 317), (120, 160)])
def test_cap_off_is_the_oracle(h, w):
    e = io.mineig(K.band_noise(h, w, 0.08, 1), 7)
    mask = np.ones((h, w), np.uint8); mask[h // 3:h // 2, w // 4:w // 2] = 0
    for md in (0, 3, 5, 7, 10):
        for m in (None, mask):
            want, ncand = io.select_corners(e, 300, 0.01, md, mask=m)
            got, (acc, exam), ranks = R.select(e, 300, 0.01, md, mask=m)
            assert np.array_equal(got.view(np.uint32), want.reshape(-1, 2).view(np.uint32)), (h, w, md, m is not None)
            assert acc == len(want) and len(R.candidates(e, 0.01, m)) == ncand and exam == (ranks[-1] + 1 if acc == 300 else ncand)
            big = R.select(e, 300, 0.01, md, mask=m, grid=(64, 300, 0))            # a cap that cannot bind
            assert np.array_equal(big[0], got) and big[1] == (acc, exam)


def _peaks(h, w, at):
    e = np.zeros((h, w), np.float32)
    for (x, y), v in at.items():
        e[y, x] = v
    return e


def test_ties_inside_a_cell_resolve_by_descending_index():
    e = _peaks(16, 16, {(2, 2): 1.0, (5, 2): 1.0, (2, 5): 1.0, (12, 12): 0.5})
    pts, stats, _ = R.select(e, 10, 0.01, 0, grid=(8, 1, 0))
    assert pts.tolist() == [[2, 5], [12, 12]] and stats == (2, 4)
    pts, _, _ = R.select(e, 10, 0.01, 0, grid=(8, 2, 0))
    assert pts.tolist() == [[2, 5], [5, 2], [12, 12]]


def test_cap_one_keeps_one_corner_per_cell():
    rng = np.random.default_rng(3)
    e = np.zeros((32, 48), np.float32)
    e[1:-1:2, 1:-1:2] = rng.random((15, 23)).astype(np.float32) + 0.5
    pts, (acc, exam), _ = R.select(e, 1000, 0.01, 0, grid=(8, 1, 0))
    cells = (pts[:, 1].astype(int) // 8) * 6 + pts[:, 0].astype(int) // 8
    assert acc == 24 and sorted(cells.tolist()) == list(range(24))
    for c in range(24):                                          # and it is the cell's strongest
        y0, x0 = 8 * (c // 6), 8 * (c % 6)
        x, y = pts[list(cells).index(c)].astype(int)
        assert e[y, x] == e[y0:y0 + 8, x0:x0 + 8].max()
    assert exam < len(R.candidates(e, 0.01))                     # the pass stopped when the last cell filled


def test_occupancy_closes_cells_and_ignores_points_outside():
    e = _peaks(16, 16, {(2, 2): 1.0, (12, 2): 0.9, (2, 12): 0.8, (12, 12): 0.7})
    occ = [(1.5, 1.5), (3.0, 7.9), (-4.0, 2.0), (16.0, 2.0), (12.0, -1.0), (12.0, 16.5), (np.nan, 3.0)]
    pts, stats, _ = R.select(e, 10, 0.01, 0, grid=(8, 2, 0), occ_pts=occ)
    assert pts.tolist() == [[12, 2], [2, 12], [12, 12]] and stats == (3, 4)     # two points closed the first cell, the rest count nowhere
    pts, _, _ = R.select(e, 10, 0.01, 0, grid=(8, 3, 0), occ_pts=occ)
    assert len(pts) == 4
    assert R.occupancy(16, 16, 8, occ).tolist() == [2, 0, 0, 0]
    assert R.occupancy(16, 16, 8, [(-0.5, 15.9)]).tolist() == [0, 0, 1, 0]      # the truncated position decides
    pts, stats, _ = R.select(e, 10, 0.01, 0, grid=(16, 2, 0), occ_pts=occ[:2])   # the one cell is full from the start
    assert len(pts) == 0 and stats == (0, 0)


def test_max_rank_cuts_the_list():
    e = _peaks(16, 16, {(2, 2): 1.0, (4, 2): 0.9, (12, 2): 0.8, (2, 12): 0.7, (12, 12): 0.6})
    assert R.select(e, 10, 0.01, 0, grid=(8, 1, 0))[0].tolist() == [[2, 2], [12, 2], [2, 12], [12, 12]]
    pts, stats, ranks = R.select(e, 10, 0.01, 0, grid=(8, 1, 3))
    assert pts.tolist() == [[2, 2], [12, 2]] and stats == (2, 3) and ranks.tolist() == [0, 2]
    assert R.select(e, 10, 0.01, 0, grid=(8, 1, 1))[1] == (1, 1)


def test_defaults_mean_off_and_bad_keywords_are_rejected(pkg, ofk):
    from of_amd.pipeline import PipelineConfig
    for cfg in (PipelineConfig(), PipelineConfig.node(), PipelineConfig.of_module(), PipelineConfig.evaluate_exp(), PipelineConfig.baseline_1080p()):
        assert (cfg.grid_cell, cfg.grid_cap, cfg.grid_max_rank) == (0, 0, 0) and cfg.corner_grid_setting() is None
    g = PipelineConfig(grid_cell=64, grid_cap=4, grid_max_rank=4000).corner_grid_setting()
    assert (g.cell, g.cap, g.max_rank) == (64, 4, 4000)
    d = ofk.corner_grid_setting()
    assert (d.cell, d.cap, d.max_rank) == (0, 0, 0)
    assert ofk.corner_grid_setting(0, cap=-5).cell == 0          # with the grid off the cap is not looked at
    for kw in (dict(cell=-1), dict(cell=8, cap=0), dict(cell=8, cap=-2), dict(cell=8, cap=1, max_rank=-1), dict(max_rank=-1)):
        with pytest.raises(ValueError):
            ofk.corner_grid_setting(**kw)
    with pytest.raises(TypeError):
        ofk.corner_grid_setting(size=8)
    import inspect
    from of_amd import velocity_node
    assert inspect.signature(velocity_node.optical_fusion.__init__).parameters["corner_grid"].default is None
    assert velocity_node.optical_fusion._corner_grid == {}


def test_the_grid_takes_the_corners_off_the_object():
    q = K.QUALITY_SCENE
    e = K.eig_of("quality", q["block"])
    y0, x0, bh, bw = q["box"]

    def share(p):
        return float(((p[:, 0] >= x0) & (p[:, 0] < x0 + bw) & (p[:, 1] >= y0) & (p[:, 1] < y0 + bh)).mean())
    plain = R.select(e, q["max_corners"], q["quality"], q["min_distance"])[0]
    grid = R.select(e, q["max_corners"], q["quality"], q["min_distance"], grid=q["grid"])[0]
    assert bh * bw / (q["h"] * q["w"]) == pytest.approx(0.15, abs=0.005)
    print(f"share of the corners on the object: plain {share(plain):.3f}, grid {share(grid):.3f}")
    assert share(plain) > 0.4 and share(grid) < 0.4 and len(grid) == q["max_corners"]
