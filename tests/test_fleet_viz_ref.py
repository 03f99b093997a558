"""CPU-only: the NumPy restatement of the fleet picture (tests/fleet_viz_ref.py) held to hand-worked facts on a 16 x 20
background with three robots, and to the particle picture's restatement for one robot.  tests/test_fleet_viz.py then
holds the device to the restatement.

The geometry the facts use (tests/test_viz_ref.py works them out): a particle at mlState (x, y) with heading 0 has
pt = ((int)x, (int)(16 - y)) and draws Arrow((-5, 0), (5, 0)) there, whose middle row covers pt.x - 6 .. pt.x + 6; a
particle left of the image draws its dot at (5, pt.y), the 21 pixels within sqrt(5) of it."""
import numpy as np
import pytest
import fleet_viz_ref as FV
import viz_ref as V

from top_down_renderer_amd import STATE_DTYPE

H, W = 16, 20
PALETTE = np.asarray([[[10, 20, 30], [40, 50, 60], [70, 80, 90]],
                      [[11, 21, 31], [41, 51, 61], [71, 81, 91]],
                      [[12, 22, 32], [42, 52, 62], [72, 82, 92]]], np.uint8)   # [robot][arrows, dots, estimate][BGR]


@pytest.fixture(scope="module", autouse=True)
def built():
    from top_down_renderer_amd import build
    build.build()   # (the restatement's cosf / sinf are the library's host functions)


@pytest.fixture(scope="module")
def bg():
    img = np.random.default_rng(5).integers(100, 200, (H, W, 3), dtype=np.uint8)
    assert not any((img == c).all(axis=2).any() for c in PALETTE.reshape(-1, 3)) and not (img == FV.GREEN).all(axis=2).any()
    return img


def states(rows):
    st = np.zeros(len(rows), STATE_DTYPE)
    for i, (x, y, th) in enumerate(rows):
        st[i]["dx_m"], st[i]["dy_m"], st[i]["theta"], st[i]["scale"], st[i]["have_init"] = x, y, th, 1.0, 1
    return st


NOBODY = {"st": states([])}
ARROW_AT_10_7 = {"st": states([(10.5, 8.5, 0.0)])}
ARROW_AT_6_7 = {"st": states([(6.5, 8.5, 0.0)])}
DOT_AT_5_7 = {"st": states([(-3.0, 8.5, 0.0)])}


def colour(img, x, y):
    return tuple(int(v) for v in img[y, x])


def pal(r, layer):
    return tuple(int(v) for v in PALETTE[r, layer])


def test_identical_particles_show_the_higher_index(bg):
    img = FV.render([ARROW_AT_10_7, ARROW_AT_10_7, NOBODY], bg, PALETTE)
    arrows, _ = V.particle_planes(ARROW_AT_10_7["st"], H, W)
    assert arrows[7, 4:17].all() and arrows.sum() == 43                # the whole stamp is inside the image
    assert (img[arrows] == PALETTE[1, 0]).all()                        # robot 1's colour on every pixel of the arrow
    assert (img[~arrows] == bg[~arrows]).all()
    swapped = FV.render([NOBODY, ARROW_AT_10_7, ARROW_AT_10_7], bg, PALETTE)
    assert (swapped[arrows] == PALETTE[2, 0]).all()


def test_dot_of_robot_0_lies_over_arrow_of_robot_2(bg):
    img = FV.render([DOT_AT_5_7, NOBODY, ARROW_AT_6_7], bg, PALETTE)
    assert colour(img, 5, 7) == pal(0, 1) and colour(img, 3, 7) == pal(0, 1) and colour(img, 7, 7) == pal(0, 1)
    assert colour(img, 2, 7) == pal(2, 0) and colour(img, 8, 7) == pal(2, 0)   # beside the dot the arrow shows
    _, dots = V.particle_planes(DOT_AT_5_7["st"], H, W)
    assert dots.sum() == 21 and (img[dots] == PALETTE[0, 1]).all()


def test_estimate_of_robot_0_lies_over_dot_of_robot_2(bg):
    est = {"st": states([]), "best": (5.5, 8.5, 0.0)}                  # the max-likelihood arrow at pt (5, 7)
    img = FV.render([est, NOBODY, DOT_AT_5_7], bg, PALETTE)
    assert colour(img, 5, 7) == pal(0, 2) and colour(img, 3, 7) == pal(0, 2)
    assert colour(img, 5, 5) == pal(2, 1)                              # the dot's top pixel, which the arrow misses
    assert colour(img, 11, 7) == pal(0, 2) and colour(img, 12, 7) == tuple(bg[7, 12])


def test_callers_arrow_lies_over_everything(bg):
    est = {"st": states([(10.5, 8.5, 0.0)]), "best": (5.5, 8.5, 0.0)}
    robots = [est, DOT_AT_5_7, ARROW_AT_6_7]
    img = FV.render(robots, bg, PALETTE, arrows=[[2, 7, 9, 7]])
    for x in range(1, 11):
        assert colour(img, x, 7) == FV.GREEN, x
    without = FV.render(robots, bg, PALETTE)
    assert colour(without, 5, 7) == pal(0, 2)                          # estimate over dot over arrow beneath it
    assert colour(img, 5, 5) == pal(1, 1) and colour(img, 16, 7) == pal(0, 0)


@pytest.mark.parametrize("s", [1.0, 0.5, 1.7])
def test_one_robot_in_the_classic_colours_is_the_particle_picture(bg, s):
    rng = np.random.default_rng(9)
    st = states([(x, y, th) for x, y, th in zip(rng.uniform(-4, 24, 40), rng.uniform(-4, 20, 40), rng.uniform(-7, 7, 40))])
    means, covs = [[8.0, 8.0, 0.7]], [[[9.0, 2.0, 0], [2.0, 4.0, 0], [0, 0, 1]]]
    best, arrows = (12.5, 6.5, 2.0), [[1, 1, 15, 12]]
    got = FV.render([{"st": st, "means": means, "covs": covs, "best": best}], bg, [FV.CLASSIC], arrows, s)
    want = V.render(st, bg, means, covs, best, arrows, s)
    assert got.shape == want.shape and np.array_equal(got, want)
    p0, p1, p2 = FV.robot_planes({"st": st, "means": means, "covs": covs, "best": best}, H, W)
    assert p0.any() and p1.any() and p2.any()
