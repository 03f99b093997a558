"""What the fleet picture (include/tdr.h, "the fleet picture") must be, restated in NumPy on top of the
particle picture's restatement (tests/viz_ref.py: the planes, the overlay, the published size and the resample are that
module's, unchanged).  New here: the palette and the composition over robots — layer-major, the highest index wins.
Shared by tests/test_fleet_viz_ref.py and tests/test_fleet_viz.py; not a test module, and nothing here imports the
package's kernels."""
import numpy as np
from viz_ref import overlay, particle_planes, published_size, resample, segment_planes

GREEN = (0, 255, 0)
CLASSIC = ((0, 0, 255), (0, 255, 0), (255, 0, 0))   # one robot's colours in the particle picture: arrows, dots, estimate


def robot_planes(robot, H, W):
    """(arrows, dots, estimate) of one robot as bool (H, W) arrays.  robot: dict with st, and optionally means, covs,
    best ({x, y, theta} of the max-likelihood state, after the first update)."""
    p0, p1 = particle_planes(robot["st"], H, W)
    p2, _ = segment_planes(overlay(robot.get("means", ()), robot.get("covs", ()), robot.get("best"), None, H), H, W)
    return p0, p1, p2


def compose(background, planes, palette, green):
    """Layer-major over robots: arrows of robots 0 .. k-1, then dots, then estimates, then the caller's green plane; a
    later assignment overwrites, so within a layer the highest index shows."""
    img = np.array(background, np.uint8, copy=True)
    pal = np.asarray(palette, np.uint8).reshape(len(planes), 3, 3)
    for layer in range(3):
        for r, p in enumerate(planes):
            img[p[layer]] = pal[r, layer]
    img[green] = GREEN
    return img


def render(robots, background, palette, arrows=None, pub_scale=1.0):
    """The published fleet image."""
    H, W = background.shape[:2]
    out_h, out_w = published_size(H, W, pub_scale)
    if not (1 <= out_h <= 32768 and 1 <= out_w <= 32768):
        raise ValueError("no published image")
    planes = [robot_planes(r, H, W) for r in robots]
    _, green = segment_planes(overlay((), (), None, arrows, H), H, W)
    return resample(compose(background, planes, palette, green), out_h, out_w)
