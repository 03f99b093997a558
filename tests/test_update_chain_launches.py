"""tdr_k_update_weights and tdr_k_prefix above 32 768 weights with fewer launches (csrc/tdr_filter.hip, tdr_prefix.hip): the
counting passes leave the chains' chunk sums (and one count per chunk, in the scratch behind the statistics), and a chain's
head runs beside the summaries of the chunks behind it.  None of that may show: `sum`, `mean`, `bottom_stddev`
are the oracle's serial float chains bit for bit, the counts and the argmax are exact NumPy, the weights the oracle's within
its 1e-6, the running sum and maximum NumPy's serial float32 chain bit for bit — with the heads on and off, and several
times in a row on one scratch buffer (the chunk sums and counts a call leaves there are not the next call's)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

f32 = np.float32
# one weight past the one-workgroup form; one past a chunk (4096) behind it: a last chunk of one weight; whole chunks; a
# ragged tail and more chunks (25) than the head takes (8)
SIZES = [32_769, 36_865, 65_536, 100_003]
KINDS = ["nan and zeros", "bulk ties", "head sums to zero", "lognormal"]


@pytest.fixture(scope="module")
def k():
    import torch
    from top_down_renderer_amd.kernels import HipKernels

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return HipKernels()


def _weights(kind, n):
    rng = np.random.default_rng(KINDS.index(kind) * 1000 + n % 977)
    if kind == "nan and zeros":
        raw = (1.0 / (rng.random(n) * 20 + 0.15)).astype(f32)
        raw[rng.random(n) < 0.05] = np.nan
        raw[rng.random(n) < 0.03] = 0.0
        raw[4096:8192] = np.nan          # a whole chunk without a valid weight
    elif kind == "bulk ties":
        raw = np.full(n, f32(1.0), f32)
        raw[::2] = f32(1.0 + 2.0 ** -23)  # half-ulp ties against a growing sum
        raw[rng.random(n) < 0.3] = f32(3.25)
    elif kind == "head sums to zero":
        raw = np.zeros(n, f32)
        raw[32_768:] = rng.random(n - 32_768).astype(f32) + f32(0.01)
    else:
        raw = np.exp(rng.normal(0, 3, n)).astype(f32)
        raw[rng.random(n) < 0.02] = np.nan
    ld = (rng.random(n) * 0.4).astype(f32)
    return raw, ld


_REF = {}


def _reference(oracle, kind, n):
    """(raw, last_dist, oracle weights, argmax, {sum, mean, bottom}, valid count, count below the mean), computed once."""
    key = (kind, n)
    if key not in _REF:
        raw, ld = _weights(kind, n)
        with np.errstate(all="ignore"):
            w, best, stats = oracle.update_weights(raw, ld)
            nv = int(np.count_nonzero(~np.isnan(raw)))
            nu = int(np.count_nonzero(raw < f32(stats[1])))   # NaN compares false
        _REF[key] = (raw, ld, w, best, np.asarray(stats[:3], f32), nv, nu)
    return _REF[key]


def _check(k, oracle, kind, n, info, w, rm):
    import torch
    raw, ld, w_ref, best, stats, nv, nu = _reference(oracle, kind, n)
    got_info = info[:8].cpu().numpy()
    got_w = w.cpu().numpy()
    assert np.array_equal(got_info[1:4], stats, equal_nan=True), (got_info[1:4], stats)   # the chains: bit for bit
    assert (int(got_info[5]), int(got_info[6])) == (nv, nu)
    assert int(info[:1].cpu().view(torch.int32).item()) == best
    assert np.allclose(got_w, w_ref, rtol=1e-6, atol=0, equal_nan=True)
    # the argmax of the weights as written: first maximum (exact NumPy on the GPU's own weights agrees with the oracle's)
    assert int(np.argmax(np.where(np.isnan(got_w), -np.inf, got_w))) == best
    with np.errstate(all="ignore"):
        run = np.cumsum(got_w, dtype=f32)   # the serial float32 chain of particle_filter.cpp:179
    assert np.array_equal(rm.cpu().numpy(), np.maximum.accumulate(np.where(np.isnan(run), -np.inf, run)).astype(f32))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_statistics_and_running_sum_are_the_serial_chains(k, oracle, kind, n):
    raw, ld = _reference(oracle, kind, n)[:2]
    before = k.lib.tdr_config_prefix_small(-1)
    try:
        for heads in (1, 0):   # 0: no one-workgroup heads, the chunk walk (and every summary) from the first addend on
            k.lib.tdr_config_prefix_small(heads)
            w, info, rm = k.zeros((n,)), k.zeros((65536,)), k.zeros((n,))
            k.update_weights(k.to_device(raw), k.to_device(ld), n, w, info)
            k.prefix(w, n, rm)
            _check(k, oracle, kind, n, info, w, rm)
    finally:
        k.lib.tdr_config_prefix_small(before)


@pytest.mark.parametrize("n", SIZES)
def test_two_calls_in_a_row_on_one_scratch_buffer(k, oracle, n):
    """The scratch behind info[8:] keeps the chunk sums, the counts and the chain headers of a call: a second call on other
    weights, and a third on the first ones again, each give their own statistics."""
    info, w, rm = k.zeros((65536,)), k.zeros((n,)), k.zeros((n,))
    for kind in ("nan and zeros", "lognormal", "nan and zeros"):
        raw, ld = _reference(oracle, kind, n)[:2]
        info[:8].fill_(-1.0)
        k.update_weights(k.to_device(raw), k.to_device(ld), n, w, info)
        k.prefix(w, n, rm)
        _check(k, oracle, kind, n, info, w, rm)
