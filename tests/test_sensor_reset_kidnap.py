"""GPU: the closed loop of the kidnapped robot (tests/test_recovery.py::kidnap_run's scenario) with sensor resetting: every
recovery step gives the injected slots the best of 64 road candidates against the step's scan (recoveryStepSensor), under
the project's three tracker settings.  The traces are in DESIGN.md 5.17."""
import numpy as np
import pytest

from test_recovery import KIDNAP_RP, RADIUS

pytestmark = pytest.mark.gpu
CANDIDATES = 64
# alpha_slow / alpha_fast: the setting of tests/test_recovery.py and the two faster trackers of DESIGN.md 5.16, which the
# uniform injection did not recover with in 80 steps
SETTINGS = {"0.05/0.5": dict(KIDNAP_RP), "0.1/0.9": dict(KIDNAP_RP, alpha_slow=0.1, alpha_fast=0.9),
            "0.2/1.0": dict(KIDNAP_RP, alpha_slow=0.2, alpha_fast=1.0)}
# Measured on the MI355X over 80 steps after the move: the step from which the max-likelihood particle is
# within RADIUS of the new pose, step after step.  It stays there through step 77 / 58 / 55; then the weights have sunk (the
# scenario walks the cloud 0.2 px a step while the scan stands still), the tracker asks for a few slots again and a
# tournament winner on another stretch of road takes the maximum, while the cloud stays on the new pose (3872 / 2899 / 2398
# of the 4000 particles within RADIUS after 80 steps).
STEPS_NEEDED = {"0.05/0.5": 5, "0.1/0.9": 2, "0.2/1.0": 2}


@pytest.fixture(scope="module")
def K():
    import torch
    from top_down_renderer_amd.kernels import HipKernels
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return HipKernels()


def kidnap_run_sensor(K, rp, steps_after, candidates=CANDIDATES):
    """kidnap_run of tests/test_recovery.py with recovery_every = 1 and recoveryStepSensor in place of recoveryStep: 10 steps
    at the true pose of synth's c1 scene, then the scans come from a road pose at least 400 px away.  Returns (the new pose,
    per further step: distance of the max-likelihood particle to it, particles within RADIUS of it, the step's (p,
    injected))."""
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import synth
    from top_down_renderer_amd._lib import RecoveryStateC
    sc = synth.make_scene("c1", n_particles=4000)
    cfg = sc.cfg
    rng = np.random.default_rng(77)
    while True:
        pose2 = synth.pick_true_pose(sc.lab, rng, 168)
        if np.hypot(pose2[0] - sc.pose[0], pose2[1] - sc.pose[1]) >= 400:
            break
    pts2 = synth.make_scan(cfg, sc.lab, pose2, rng)
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=K)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    r = pkg.ScanRendererPolar(sc.lut, kernels=K)
    r.set_output_shape(cfg.ncls, cfg.nb, cfg.nr)
    f = pkg.ParticleFilter(len(sc.states), m, pkg.FilterParams(fixed_scale=1.0), seed=5, kernels=K, init_particles=False)
    f.set_states(synth.make_particles(cfg, sc.lab, sc.pose, np.random.default_rng(78), n=len(sc.states), uniform_frac=0.0))
    state, params = RecoveryStateC(0.0, 0.0), pkg.RecoveryParams(**rp)

    def step():
        f.propagate((0.2, 0.0), 0.0)
        f.update(r.last_scan(), None, cfg.res)
        return f.recoveryStepSensor(state, params, candidates, r.last_scan(), cfg.res)

    r.renderSemanticTopDown(sc.pts, cfg.res, cfg.ang_res)
    for s in range(10):
        step()
    ml = f.maxLikelihood()
    assert np.hypot(ml[0] - sc.pose[0], ml[1] - sc.pose[1]) < 100      # the cloud sits on the first pose
    r.renderSemanticTopDown(pts2, cfg.res, cfg.ang_res)
    trace = []
    for s in range(steps_after):
        rec = step()
        ml = f.maxLikelihood()
        st = f.get_states()
        x = st["dx_m"] * st["scale"] + st["init_x_px"]
        y = st["dy_m"] * st["scale"] + st["init_y_px"]
        trace.append((float(np.hypot(ml[0] - pose2[0], ml[1] - pose2[1])), int((np.hypot(x - pose2[0], y - pose2[1]) < RADIUS).sum()),
                      (round(rec[0], 4), rec[1])))
    return pose2, trace


def within_run(trace):
    """(the first step, 1-based, at which the max-likelihood particle is within RADIUS; the last step of the unbroken run
    of such steps that begins there), or (None, None)."""
    inside = [d < RADIUS for d, _, _ in trace]
    if True not in inside:
        return None, None
    first = inside.index(True)
    last = first
    while last + 1 < len(inside) and inside[last + 1]:
        last += 1
    return first + 1, last + 1


@pytest.mark.parametrize("name", sorted(STEPS_NEEDED))
def test_sensor_resetting_finds_the_robot_again(K, name):
    """The max-likelihood particle is within RADIUS of the new pose after twice the measured step (the convention of
    STEPS_NEEDED / STEPS_ALLOWED in tests/test_recovery.py), under all three tracker settings: the uniform injection did
    not recover with the last two in 80 steps."""
    allowed = 2 * STEPS_NEEDED[name]
    _, trace = kidnap_run_sensor(K, SETTINGS[name], allowed)
    print("kidnap trace with sensor resetting,", name, ":", within_run(trace), trace)
    assert trace[-1][0] < RADIUS and trace[-1][1] > 0, trace[-5:]
