"""Every loop variant of the two dense scoring kernels, proven to run and exact at the integer form's limits.  Run with
`pytest -m gpu`.

score_polar_su_kernel and score_cart_su_kernel choose a loop per wave and piece of work (tests/variant_scenes.py names them
and the geometry that forces each).  Per (scene, scan):
  * a COUNTED run (tdr_profile_enable(2), span 0: every particle dense): the counters of tdr_profile_variants show that
    every wave-sector / wave-segment of the kernel ran the scene's variant — every other counter of either kernel is 0 —
    or, for a scene that admits foreign variants (the general loop next to a border: the boxes that look inwards do not
    reach the guard ring), that only those occur beside it and the scene's own is the majority.  The 16 counters are printed;
  * an uncounted run: the same bits (the counters are a runtime pointer: the code object counted is the one that ships);
  * the weights are the exact reference's bit for bit (test_int_form_limits._check, form "integer"), array-equal to the
    launch with every particle through the ray-mapped kernel and, Cartesian, to the plain kernel (cart_seg_rows 0); they
    and the float kernel's lie within 1e-5 of the oracle.
tests/test_variant_scenes_ref.py shows on the CPU that the inputs are fair."""
import numpy as np
import pytest

import variant_scenes as V
from test_cart_su import _run
from test_int_form_limits import _check
from test_shift_uniform import ALL_RAY, _score_both, tdr  # noqa: F401

pytestmark = pytest.mark.gpu

_MAPS = {}


def _device_map(pkg, k, case):
    """One device map per (map, window shape): built once, shared by the scenes on it."""
    key = (case["kind"], id(case["maps"]), case["shape"])
    if key not in _MAPS:
        a, b = case["shape"]
        if case["kind"] == "polar":
            m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), case["maps"], case["mask"], kernels=k)
            assert m.dev.desc.cwords > 0
            m.samplePtsPolar((a, b), case["ang_res"])
        else:
            m = pkg.TopDownMap(pkg.Params(resolution=1.0), case["maps"], case["mask"], kernels=k)
            m.setWindow(a, b)
        _MAPS[key] = (m, case["maps"])   # (the arrays stay alive: their id is the key)
    return _MAPS[key][0]


def _check_counters(case, v):
    print(f"{case['name']}: variant counters {v}")
    own = V.POLAR_COUNTERS if case["kind"] == "polar" else V.CART_COUNTERS
    target, admits = case["target"], case["admits"]
    assert v[target] > 0, f"the scene's variant (counter {target}) never ran: {v}"
    for c in range(16):
        if c != target and c not in admits:
            assert v[c] == 0, f"counter {c} is {v[c]}: the scene is for counter {target} and admits {admits}: {v}"
    assert 2 * v[target] > sum(v[c] for c in own), f"the scene's variant is not the majority: {v}"


@pytest.mark.parametrize("scene,scan", V.CASES)
def test_variant_runs_and_is_exact(tdr, oracle, scene, scan):
    pkg, k = tdr
    case, exact, ref = V.references(oracle, scene, scan)
    m = _device_map(pkg, k, case)
    st, sc, res = case["states"], case["scan"], case["res"]
    if case["kind"] == "polar":
        dense = lambda: _score_both(pkg, k, m, sc, res, st, case["params"], span=0.0)
        ((raw_float, _), (counted, _)), v = V.counted(k, dense)
        (_, _), (uncounted, _) = dense()
        (_, _), (all_ray, _) = _score_both(pkg, k, m, sc, res, st, case["params"], span=ALL_RAY)
        ints = [counted, uncounted, all_ray]
    else:
        counted, v = V.counted(k, lambda: _run(pkg, k, m, st, sc, res, 32, 0.0))
        ints = [counted, _run(pkg, k, m, st, sc, res, 32, 0.0),         # uncounted
                _run(pkg, k, m, st, sc, res, 32, ALL_RAY),              # every particle through the ray-mapped kernel
                _run(pkg, k, m, st, sc, res, 0, 0.0)]                   # the plain kernel
        raw_float = _run(pkg, k, m, st, sc, res, 32, 0.0, mode=0)
    _check_counters(case, v)
    assert np.array_equal(ints[0], ints[1], equal_nan=True), "counting changed the weights"
    _check(case, raw_float, ints, exact, ref)
