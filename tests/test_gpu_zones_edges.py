"""GPU: the exclusion zones at the limits of every rule (the cases of tests/zones_edge_cases.py) through ofk_zones_step against
tests/zones_reference.py: mask, table, motion bits and statistics behind every step, bit for bit, no tolerance anywhere.  What makes
each case a test of its edge is asserted on the reference alone in tests/test_zones_edge_cases.py.

One-token changes of csrc/k_zones.inc that these cases catch (tried by hand): phase B's (short) unpack read unsigned (clamp, span),
rintf -> roundf in zone_shift (clamp, drift, hulls, duplicates, the small tiling zones, 4096 points), > OFK_ZONE_VERTS -> >= (hulls),
a 32-bit ex * qy in zone_inside (span), the offset's bound 2^20 -> 2^15 (drift)."""
import numpy as np
import pytest

import zones_edge_cases as ze

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zctx(ofk):
    c = ofk.Context(0, 640, 480, 3, 512, 2)
    yield c
    c.close()


@pytest.mark.parametrize("h,w", [(48, 64), (480, 640)])
def test_clamped_and_non_finite_positions(zctx, h, w):
    tables, mask = ze.run_case(zctx, ze.clamp(h, w))
    assert [int(t.stats[0]) for t in tables] == [3, 2, 0]


@pytest.mark.parametrize("variant", ["plain", "nan"])
def test_far_drift_and_saturation(zctx, variant):
    tables, _ = ze.run_case(zctx, ze.far(variant))
    assert not tables[0].zones.any()


def test_drift_to_negative_coordinates_and_refresh_there(zctx):
    tables, _ = ze.run_case(zctx, ze.drift_negative())
    assert tables[0].zones[0, 0] == 4 and tables[0].motion[0, 0] == -45002.5


def test_hulls_of_32_33_and_34_vertices(zctx):
    ze.run_case(zctx, ze.hulls())


@pytest.mark.parametrize("case", [ze.singletons, ze.duplicates, ze.one_slot, ze.link_4096, ze.radius_0, ze.span], ids=lambda f: f.__name__)
def test_extremes_of_the_setting(zctx, case):
    ze.run_case(zctx, case())


def test_keep_and_status_bytes(zctx):
    tables, _ = ze.run_case(zctx, ze.flag_bytes())
    assert [int(t.stats[4]) for t in tables] == [32, 32, 0]


@pytest.mark.parametrize("h,w", [(33, 47), (17, 65), (16, 64)])
@pytest.mark.parametrize("radius", [0, 20])
@pytest.mark.parametrize("which", ["big", "small"])
def test_mask_tiling(zctx, h, w, radius, which):
    case = ze.tiling(h, w, radius, which)
    _, mask = ze.run_case(zctx, case)
    assert not mask[case["masks"][-1] == 0].any()


def test_4096_points_per_stream(ofk):
    """The launch at the LDS limit of k_zones_update: 48 KiB of dynamic LDS beside its static arrays."""
    ctx = ofk.Context(0, 640, 480, 2, 4096, 2)
    try:
        tables, _ = ze.run_case(ctx, ze.big_count())
        assert tables[1].stats[5] == 4096 and tables[0].stats[4] == 1200
    finally:
        ctx.close()
