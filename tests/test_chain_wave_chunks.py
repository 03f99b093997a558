"""The three exact chains above 32 768 weights at wave-chunk grain (csrc/tdr_prefix.hip, "the long chains at wave-chunk
grain"): every wave-chunk of 512 addends is summarised somewhere on the chip from a predicted binade, and one wave walks
the summaries 64 at a time with the exact sum.  Whatever was predicted, `sum`, `mean` and `bottom_stddev` are the oracle's
serial float chains and the running sum / running maximum are NumPy's serial float32 chain, bit for bit and NaN for NaN;
and everything a call writes equals, bit for bit, what tdr_config_prefix_small(0) (the 4096-chunk walk from the first
addend on, an independent second evaluation) writes for the same input.

The weights themselves are compared with the oracle's within 1e-6 as everywhere else: they are exact up to the two
normalising sums, which the update forms in double (tests/test_uw_exact.py holds that statement exactly); against the
second evaluation they are compared bit for bit.

Sizes: 65 wave-chunks with a last one of one addend (32 769: the first chunk of a second round of 64 summaries); 65 full
/ 66 with a one-addend tail (33 280, 33 281); 128 full / 128 and a one-addend tail that opens a third round (65 536,
65 537); the benchmark's size, ragged (100 003)."""
import ctypes as C

import numpy as np
import pytest

from test_update_chain_launches import k  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

f32 = np.float32
WC = 512   # addends per wave-chunk
SIZES = [32_769, 33_280, 33_281, 65_536, 65_537, 100_003]
DUAL_SLOTS = 32   # UWG_DUAL_SLOTS: crossing chunks summarised lane by lane; one more is simply carried through


def _crossing(n, c, rng):
    """Positive weights whose serial float32 sum crosses a binade inside wave-chunk c (checked here, on the CPU)."""
    x = rng.random(n) + 0.5
    at = min(c * WC + WC // 2, n - 1)
    target = np.cumsum(x)[at] - 0.5 * x[at]   # 2^20 falls inside the step of addend `at`
    x = (x * (2.0 ** 20 / target)).astype(f32)
    run = np.cumsum(x, dtype=f32)
    lo, hi = c * WC, min((c + 1) * WC, n) - 1
    assert np.frexp(run[lo - 1])[1] + 1 == np.frexp(run[hi])[1], "the arrangement must cross in the chunk"
    return x


def _doubling(n):
    """Dyadic weights that double the sum in every wave-chunk from chunk 20 on: more crossing chunks than dual slots."""
    x = np.zeros(n, f32)
    last = min(95, (n - 1) // WC)
    assert last - 20 > DUAL_SLOTS
    for c in range(20, last + 1):
        x[c * WC:(c + 1) * WC] = f32(2.0 ** (-40 + max(c - 21, 0)))
    return x


def _make(kind, n):
    rng = np.random.default_rng(CONTENTS.index(kind) * 7919 + n)
    if kind == "lognormal":
        return np.exp(rng.normal(0, 3, n)).astype(f32)
    if kind == "all equal":
        return np.full(n, f32(0.7), f32)
    if kind == "half-ulp spam":
        x = np.full(n, f32(1.0), f32)   # half an ulp of the sum: every addition is a tie that falls back
        x[0] = f32(2.0 ** 24)
        x[rng.random(n) < 0.001] = f32(3.0)
        return x
    if kind == "zero head":
        x = np.zeros(n, f32)
        x[min(40_000, n - 1):] = (rng.random(n - min(40_000, n - 1)) + 0.01).astype(f32)
        return x
    if kind.startswith("crossing in chunk "):
        return _crossing(n, int(kind.split()[-1]), rng)
    if kind == "doubling":
        return _doubling(n)
    if kind == "nan 5%":
        x = np.exp(rng.normal(0, 2, n)).astype(f32)
        x[rng.random(n) < 0.05] = np.nan
        return x
    if kind in ("one negative", "one inf", "inf then -inf"):
        x = (rng.random(n) + 0.25).astype(f32)
        at = 33_000 if n > 33_001 else n - 2
        if kind == "one negative":
            x[at] = f32(-3.5)
        elif kind == "one inf":
            x[at] = np.inf
        else:
            x[at], x[at + 1] = np.inf, -np.inf
        return x
    assert kind == "subnormals"
    x = (rng.integers(1, 1000, n).astype(np.uint32)).view(f32).copy()   # the bit patterns 1 .. 999: subnormal floats
    x[n // 2:] = np.exp(rng.normal(0, 2, n - n // 2)).astype(f32)
    return x


CONTENTS = ["lognormal", "all equal", "half-ulp spam", "zero head", "crossing in chunk 63", "crossing in chunk 64",
            "crossing in chunk 65", "doubling", "nan 5%", "one negative", "one inf", "inf then -inf", "subnormals"]


def _exists(kind, n):
    if kind.startswith("crossing in chunk "):
        return int(kind.split()[-1]) <= (n - 1) // WC   # 32 769 and 33 280 have no chunk 65
    return True


CASES = [(kind, n) for kind in CONTENTS for n in SIZES if _exists(kind, n)]
_REF = {}


def _reference(oracle, kind, n):
    """(weights, last_dist, the oracle's update, NumPy's serial running sum and maximum of the weights), computed once."""
    if (kind, n) not in _REF:
        x = _make(kind, n)
        ld = (np.random.default_rng(n).random(n) * 0.4).astype(f32)
        with np.errstate(all="ignore"):
            w, best, stats = oracle.update_weights(x, ld)
            run = np.cumsum(x, dtype=f32)   # the serial float32 chain of particle_filter.cpp:179
            rmax = np.maximum.accumulate(np.where(np.isnan(run), -np.inf, run)).astype(f32)
        for a in (w, run, rmax):
            a.setflags(write=False)
        _REF[(kind, n)] = (x, ld, w, np.asarray(stats[:3], f32), run, rmax)
    return _REF[(kind, n)]


def _run(k, x, ld, n, info, ws):
    """One update and one running sum (tdr_k_prefix_mode 2) of x: info[:8] and weights, sums and maxima, as bytes."""
    xd = k.to_device(x)
    w, rm, pf = k.zeros((n,)), k.zeros((n,)), k.zeros((n,))
    info[:8].fill_(-1.0)
    k.update_weights(xd, k.to_device(ld), n, w, info)
    assert k.lib.tdr_k_prefix_mode(C.c_void_p(xd.data_ptr()), n, 2, C.c_void_p(rm.data_ptr()), C.c_void_p(pf.data_ptr()),
                                   C.c_void_p(ws.data_ptr()), k.stream()) == 0
    return info[:8].cpu().numpy(), w.cpu().numpy(), pf.cpu().numpy(), rm.cpu().numpy()


def _check(k, oracle, kind, n, info, ws):
    x, ld, w_ref, stats, run, rmax = _reference(oracle, kind, n)
    before = k.lib.tdr_config_prefix_small(-1)
    got = {}
    try:
        for on in (1, 0):
            k.lib.tdr_config_prefix_small(on)
            got[on] = _run(k, x, ld, n, info, ws)
    finally:
        k.lib.tdr_config_prefix_small(before)
    for on in (1, 0):   # the CPU's serial chains
        g_info, g_w, g_pf, g_rm = got[on]
        assert np.array_equal(g_info[1:4], stats, equal_nan=True), (on, g_info[1:4], stats)
        assert np.allclose(g_w, w_ref, rtol=1e-6, atol=0, equal_nan=True), on
        assert np.array_equal(g_pf, run, equal_nan=True), on
        assert np.array_equal(g_rm, rmax), on
    for a, b in zip(got[1], got[0]):   # the second evaluation, everything written
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("kind,n", CASES)
def test_chains_are_the_serial_chains_at_every_size(k, oracle, kind, n):  # noqa: F811
    info = k.zeros((65536,))
    _check(k, oracle, kind, n, info, k.empty((int(k.lib.tdr_prefix_workspace_bytes(n)),), _u8()))


def _u8():
    import torch
    return torch.uint8


def test_two_calls_in_a_row_with_different_sizes_on_one_workspace(k, oracle):  # noqa: F811
    """The wave-chunk records, the dual slots and the flags of a call stay in the workspace: a call on fewer weights, on
    more, and on an input that takes the 4096-chunk path reads none of them."""
    info = k.zeros((65536,))
    ws = k.empty((int(k.lib.tdr_prefix_workspace_bytes(max(SIZES))),), _u8())
    for kind, n in (("lognormal", 100_003), ("crossing in chunk 64", 33_281), ("one negative", 65_537),
                    ("all equal", 65_536), ("doubling", 100_003), ("lognormal", 32_769)):
        _check(k, oracle, kind, n, info, ws)


def test_workspace_grows_only_above_the_one_workgroup_sizes(k):  # noqa: F811
    """Up to 32 768 weights the workspace is the chunk headers alone, as before; above, the records follow."""
    lib = k.lib
    assert lib.tdr_prefix_workspace_bytes(32_768) == 8 * 32
    n = 32_769
    nch, nwc = 9, 65
    assert lib.tdr_prefix_workspace_bytes(n) >= nch * 32 + nwc * 24 + nch * 4 + DUAL_SLOTS * 1024
