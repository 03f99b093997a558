"""The inputs of tests/test_loop_variants.py are fair before any kernel sees them (CPU only): for every scene of
tests/variant_scenes.py and every scan it is scored with,
  * the launch has an integer form by the device's own rules (int_form_cases.int_form_expected);
  * the exact reference (tests/int_exact_ref.py) and the oracle agree to 1e-5 with the same NaN and zero pattern;
  * at least half of the particles have a finite non-zero weight;
  * the all-known scenes have an all-zero mask under every window (int_form_cases.window_of).
Conditions on the inputs: the seeds of variant_scenes.make_case are those for which the references alone satisfy them."""
import numpy as np
import pytest

import int_form_cases as T
import variant_scenes as V


@pytest.mark.parametrize("scene,scan", V.CASES)
def test_scene_is_fair(oracle, scene, scan):
    case, exact, ref = V.references(oracle, scene, scan)
    assert len(case["states"]) == V.SCENES[scene]["n"] and case["form"] == "integer"
    assert T.int_form_expected(case["scan"], case["maps"])
    assert np.array_equal(np.isnan(exact), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.array_equal(exact[ok] == 0, ref[ok] == 0)
    err = np.abs(exact[ok].astype(np.float64) - ref[ok]) / np.maximum(np.abs(ref[ok]), 1e-30)
    assert err.max(initial=0.0) <= 1e-5, err.max()
    live = np.isfinite(exact) & (exact != 0)
    assert 2 * int(live.sum()) >= len(exact), int(live.sum())
    if scene == "far_nan":   # the NaN particle alone has no weight; its 63 neighbours in the wave do
        assert np.isnan(exact[V.NAN_PARTICLE]) and int(live.sum()) == len(exact) - 1
    if case["all_known"]:
        for st in case["states"]:
            assert not T.window_of(oracle, case, st)[1].any()
