"""CPU-only: the NumPy restatement of the particle picture (tests/viz_ref.py) held to hand-worked facts, and the
library's two host functions of the definition (tdr_viz_arrow_host, tdr_viz_overlay_host) held to the restatement,
integer for integer.  tests/test_viz.py then holds the device to the restatement."""
import math

import numpy as np
import pytest
import viz_ref as V

from top_down_renderer_amd import STATE_DTYPE

F32 = np.float32


def states(rows):
    """rows of (x, y, theta): particles at mlState (x, y) with scale 1 and init 0."""
    st = np.zeros(len(rows), STATE_DTYPE)
    for i, (x, y, th) in enumerate(rows):
        st[i]["dx_m"], st[i]["dy_m"], st[i]["theta"], st[i]["scale"], st[i]["have_init"] = x, y, th, 1.0, 1
    return st


@pytest.fixture(scope="module")
def reachable():
    from top_down_renderer_amd import build
    build.build()
    sweep = np.linspace(-4 * math.pi, 4 * math.pi, 2_000_001).astype(F32)
    return np.unique(V.dirs(sweep), axis=0)


def test_arrow_of_the_horizontal_heading_by_hand():
    segs = V.arrow(-5, 0, 5, 0)
    assert segs == [(-5, 0, 5, 0), (3, -2, 5, 0), (3, 2, 5, 0)]
    st = V.arrow_stamp(5, 0)
    assert len(st) == 43
    assert [int((st[:, 1] == y).sum()) for y in range(-3, 4)] == [1, 3, 11, 13, 11, 3, 1]


def test_exactly_28_directions_within_6_pixels(reachable):
    assert len(reachable) == 28
    assert [0, 0] not in reachable.tolist()
    for dx, dy in reachable:
        assert np.abs(V.arrow_stamp(dx, dy)).max() <= 6


def test_arrow_shapes_do_not_depend_on_where_they_are(reachable):
    """A particle's arrow is the tabulated Arrow(-dir, dir) moved to pt: no tip coordinate is near enough to a half for the
    double sum p2 + tip cos(...) to round another way at any pt an image can hold."""
    for dx, dy in reachable.tolist():
        ang, tip = math.atan2(-2 * dy, -2 * dx), math.hypot(2 * dx, 2 * dy) * 0.3
        for a in (ang + math.pi / 4, ang - math.pi / 4):
            for v in (dx + tip * math.cos(a), dy + tip * math.sin(a)):
                assert abs(v - math.floor(v) - 0.5) > 1e-6
        for px, py in ((32768, 32768), (1000, 7)):
            moved = [(x1 + px, y1 + py, x2 + px, y2 + py) for x1, y1, x2, y2 in V.arrow(-dx, -dy, dx, dy)]
            assert V.arrow(px - dx, py - dy, px + dx, py + dy) == moved


def test_disc_has_21_pixels():
    assert len(V.DISC) == 21 and len({tuple(p) for p in V.DISC.tolist()}) == 21


def test_conversions_follow_x86():
    for v in (float("nan"), float("inf"), float("-inf"), 3e9, -3e9):
        assert V.f2i(v) == V.INT_MIN
        assert min(max(V.f2i(v), 5), 40 - 5) == 5
    assert V.f2i(-0.9) == 0 and V.f2i(2.9) == 2 and V.f2i(-2.9) == -2
    assert V.f2i_array(np.asarray([np.nan, 3e9, -3e9, 7.5, -2147483648.0], F32)).tolist() == [V.INT_MIN] * 3 + [7, V.INT_MIN]


def test_inside_rule_keeps_the_reference_comparison():
    H, W = 40, 50
    bg = np.zeros((H, W, 3), np.uint8)
    # pt.x = W is inside: an arrow, clipped to its pixels left of the edge
    a, d = V.particle_planes(states([(W, 20, 0.0)]), H, W)
    assert a.any() and not d.any() and a[:, : W - 6].sum() == 0
    # pt.x = W + 1 is a dot at W - 5
    a, d = V.particle_planes(states([(W + 1, 20, 0.0)]), H, W)
    assert not a.any() and d.sum() == 21 and d[H - 20, W - 5]
    # non-finite coordinates: a dot at 5
    for bad in (float("nan"), float("inf"), float("-inf"), 1e20):
        a, d = V.particle_planes(states([(bad, bad, 0.0)]), H, W)
        assert not a.any() and d.sum() == 21 and d[5, 5]
    # a non-finite heading leaves the image unchanged
    for th in (float("nan"), float("inf")):
        assert np.array_equal(V.render(states([(20, 20, th)]), bg), bg)


def test_resample_identity_and_checkerboard():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (12, 14, 3), dtype=np.uint8)
    assert np.array_equal(V.resample(img, 12, 14), img)
    small = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)
    blocks = np.repeat(np.repeat(small, 2, axis=0), 2, axis=1)      # constant on 2 x 2 cells
    assert V.published_size(12, 14, 0.5) == (6, 7)
    assert np.array_equal(V.resample(blocks, 6, 7), small)


def test_published_size():
    assert V.published_size(4000, 4000, 0.2) == (800, 800)
    assert V.published_size(37, 29, 0.37) == (13, 10)
    assert V.published_size(37, 29, float("nan")) == (V.INT_MIN, V.INT_MIN)
    assert V.published_size(37, 29, 0.01) == (0, 0)


def test_host_arrow_matches_the_restatement(reachable):
    from top_down_renderer_amd.kernels import viz_arrow_host
    for dx, dy in reachable.tolist():
        assert viz_arrow_host(dx, dy).tolist() == [list(s) for s in V.arrow(-dx, -dy, dx, dy)]


MIX_MEANS = np.asarray([[20.5, 30.25, 0.3], [40, 40, 1.0], [50, 50, 2.0]], F32)
MIX_COVS = np.asarray([[[30, 5, 0], [5, 12, 0], [0, 0, 1]],
                       [[1, 5, 0], [5, 1, 0], [0, 0, 1]],        # not PSD: nothing from it or after it
                       [[9, 0, 0], [0, 9, 0], [0, 0, 1]]], F32)


def test_host_overlay_matches_the_restatement():
    from top_down_renderer_amd.kernels import viz_overlay_host
    arrows = [[1, 2, 30, 40], [-20, 5, 90, 5], [3_000_000, 0, 5, 5]]   # the last one is out of range: not drawn
    got = viz_overlay_host(MIX_MEANS, MIX_COVS, [10.5, 11.5, 0.5], arrows, 64)
    want = V.overlay(MIX_MEANS, MIX_COVS, [10.5, 11.5, 0.5], arrows, 64)
    assert got.tolist() == [list(s) for s in want]
    assert len(want) == 75 + 3 + 6                     # one component (72 edges + its arrow), best, two caller's arrows
    # all three components once the second is PSD; a degenerate ellipse; no best state; non-finite values
    covs = MIX_COVS.copy()
    covs[1] = [[0.5, 0, 0], [0, 0.25, 0], [0, 0, 1]]             # (int)sqrt = 0: an ellipse of size 0
    assert len(V.overlay(MIX_MEANS, covs, None, None, 64)) == 3 * 75
    assert viz_overlay_host(MIX_MEANS, covs, None, None, 64).tolist() == [list(s) for s in V.overlay(MIX_MEANS, covs, None, None, 64)]
    means = MIX_MEANS.copy()
    means[0, 0], means[2, 2] = np.nan, np.inf
    covs[2, 0, 0] = 1e30
    assert viz_overlay_host(means, covs, [np.nan, 1, 2], None, 64).tolist() == [list(s) for s in V.overlay(means, covs, [np.nan, 1, 2], None, 64)]
    assert viz_overlay_host(np.zeros((0, 3)), np.zeros((0, 3, 3)), None, None, 64).shape == (0, 5)
