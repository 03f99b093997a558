"""The integer form of a scoring launch at the magnitude limits it sets itself, against an exact sum.  Run with `pytest -m gpu`.

The form's claim (README.md): class sums are exact integers, rounded to float once, and a weight does
not depend on the kernel, split or rank that formed it.  tests/int_exact_ref.py states that weight on the CPU with every
sum formed exactly; tests/int_form_cases.py holds the launches: counts up to 2^24 - 1 (descriptor against list, the
Cartesian block descriptor's 24 count bits), bins of several large classes, a list entry for every bin, class totals past
2^53 (where rounding through a double is rounding twice), a dictionary whose largest integer is just below 2^32 with class
sums close to 2^64, and the bound on the scan's total count ("mass bound", int_form_off) on both sides of 2^24 — and at
2^32, where a 32-bit word that wraps reads 0.

Per case, polar (shift-uniform kernel, mixed launch, ray-mapped kernel: tests/test_shift_uniform.py::_score_both, shards of
a filter of 10^6) and Cartesian (plain kernel, generated loop, mixed, ray-mapped: tests/test_cart_su.py::_run):
  * the integer launches are array-equal;
  * "integer" cases: the weights are the exact reference's, bit for bit;
  * "float" cases (the device must notice that the scan or the map has no integer form): the bits of the float kernel;
  * always: within 1e-5 of the oracle with its NaN and zero pattern (BASELINE.json north_star) — the float kernel too.
The float kernel's distance from the exact reference is printed, not bounded (DESIGN.md 3 records it); so are the loop
variants the dense kernels ran (tdr_profile_variants) — tests/test_loop_variants.py is where each variant is demanded.
None of these inputs indexes memory with a count: a failure here is a wrong number."""
import numpy as np
import pytest

import int_form_cases as T
from test_cart_su import _run
from test_shift_uniform import ALL_RAY, _score_both, tdr  # noqa: F401
from variant_scenes import counted

pytestmark = pytest.mark.gpu


def _rel(w, ref):
    ok = ~np.isnan(ref)
    return float((np.abs(w[ok].astype(np.float64) - ref[ok]) / np.maximum(np.abs(ref[ok]), 1e-30)).max(initial=0.0))


def _same_pattern(w, ref):
    assert np.array_equal(np.isnan(w), np.isnan(ref)), (int(np.isnan(w).sum()), int(np.isnan(ref).sum()))
    ok = ~np.isnan(ref)
    assert np.array_equal(w[ok] == 0, ref[ok] == 0)


def _check(case, raw_float, ints, exact, ref):
    """raw_float: the float kernel's weights (mode 0); ints: the weights of the launches in mode 2."""
    got = ints[0]
    for kind, w in (("float kernel", raw_float), ("mode 2", got)):
        if np.array_equal(np.isnan(w), np.isnan(ref)):
            print(f"{case['name']} {case['kind']} [{case['form']} form] {kind}: max relative deviation from the exact "
                  f"reference {_rel(w, exact):.3e}, from the oracle {_rel(w, ref):.3e}")
        else:
            print(f"{case['name']} {case['kind']} [{case['form']} form] {kind}: NaN pattern differs from the oracle's")
    for other in ints[1:]:
        assert np.array_equal(got, other, equal_nan=True), f"{int((got != other).sum())} weights differ between launches"
    if case["form"] == "integer":
        _same_pattern(got, exact)
        ok = ~np.isnan(exact)
        differ = got[ok].view(np.uint32) != exact[ok].view(np.uint32)
        assert not differ.any(), f"{int(differ.sum())} weights are not the exact reference's bits; off by {_rel(got, exact):.3e}"
    else:
        assert np.array_equal(got, raw_float, equal_nan=True), "the integer kernels ran on a launch that has no integer form"
    for w in (got, raw_float):
        _same_pattern(w, ref)
        assert _rel(w, ref) <= 1e-5, f"max rel err {_rel(w, ref):.3e}"


@pytest.mark.parametrize("name", T.NAMES)
def test_polar_launch_at_the_limits(tdr, oracle, name):
    pkg, k = tdr
    case, exact, ref = T.references(oracle, name, "polar")
    nb, nr = case["shape"]
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), case["maps"], case["mask"], kernels=k)
    assert m.dev.desc.cwords > 0
    tail = m.dev.dict.cpu().numpy()[2048:2050].view(np.uint32)      # the dictionary as integers: q, "has an integer form"
    assert int(tail[1]) == (0 if name == "dictionary_at_2p32" else 1) and (int(tail[0]) == 23 or not tail[1])
    m.samplePtsPolar((nb, nr), case["ang_res"])
    runs = []
    for span in (0.0, 3.0, ALL_RAY):
        r, v = counted(k, lambda: _score_both(pkg, k, m, case["scan"], case["res"], case["states"], case["params"], span=span,
                                              ctx=k.score_ctx_create() if span == 3.0 else None))
        print(f"{name} polar, span {span:g}: variant counters {v}")     # which loops of the dense kernel the case reached
        runs.append(r)
    floats = [r[0][0] for r in runs]
    assert all(np.array_equal(floats[0], f, equal_nan=True) for f in floats[1:])
    _check(case, floats[0], [r[1][0] for r in runs], exact, ref)


@pytest.mark.parametrize("name", T.NAMES)
def test_cartesian_launch_at_the_limits(tdr, oracle, name):
    pkg, k = tdr
    case, exact, ref = T.references(oracle, name, "cart")
    rows, cols = case["shape"]
    m = pkg.TopDownMap(pkg.Params(resolution=1.0), case["maps"], case["mask"], kernels=k)
    m.setWindow(rows, cols)
    st, scan, res = case["states"], case["scan"], case["res"]
    dense, v_dense = counted(k, lambda: _run(pkg, k, m, st, scan, res, 32, 0.0))     # every particle dense, the generated loop
    mixed, v_mixed = counted(k, lambda: _run(pkg, k, m, st, scan, res, 32, 3.0))
    print(f"{name} cart: variant counters, every particle dense {v_dense}, mixed launch {v_mixed}")
    ints = [dense,
            _run(pkg, k, m, st, scan, res, 0, 0.0),         # ... the plain kernel
            mixed,
            _run(pkg, k, m, st, scan, res, 32, ALL_RAY)]    # every particle through the ray-mapped kernel
    _check(case, _run(pkg, k, m, st, scan, res, 32, 0.0, mode=0), ints, exact, ref)
