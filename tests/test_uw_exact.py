"""tdr_k_update_weights held to the exact statement of the update (tests/uw_exact_ref.py; tests/test_uw_exact_ref.py ties
that statement to the oracle): NaN fill or all-ones fallback, first normalisation, travel-distance blend, second
normalisation and first-maximum argmax are a fixed sequence of correctly rounded float operations but for the order of two
double sums, so the weights have the bits of one of at most four candidates.  On every path — one workgroup wave by wave
(default) and chunk by chunk (tdr_config_uw_waves(0)) up to 32 768 weights, the multi-workgroup passes with and without the
one-workgroup heads (tdr_config_prefix_small) above — at the smallest sizes around every structure of those kernels, and on
weights that reach the fallback either way, overflow `sum` or `bottom_stddev`, are subnormal, negative, infinite or tied.

The batched kernel runs the same body; tests/test_batch*.py tie it byte for byte to the standalone call.

The host model of a case is computed once per process (uw_exact_ref.model).  Nearly all of the file's time is the device's,
on the weights whose chains overflow, hold an infinity or are subnormal: up to half a second per call at 100 003 weights
(measured; presumably the chains adding element by element where they cannot predict a chunk).  The other cases take
microseconds."""
import numpy as np
import pytest

import uw_exact_ref as X

pytestmark = pytest.mark.gpu

f32 = np.float32
TIE_SIZES = (513, 1025, 4097, 20_000, 32_768, 32_769, 65_537, 100_003)


@pytest.fixture(scope="module")
def k():
    import torch
    from top_down_renderer_amd.kernels import HipKernels

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return HipKernels()


def _both_paths(k, raw, ld):
    """[(weights, info[:8], argmax)] of the two paths of this size, the default one first; the switch is put back."""
    n = len(raw)
    switch = k.lib.tdr_config_uw_waves if n <= 32_768 else k.lib.tdr_config_prefix_small
    before = switch(-1)
    out = []
    try:
        d_raw, d_ld = k.to_device(np.array(raw)), k.to_device(np.array(ld))   # (copies: the model's arrays are read-only)
        for on in (1, 0):
            switch(on)
            w, info = k.zeros((n,)), k.zeros((65536,))
            w.fill_(-1.0)
            info[:8].fill_(-1.0)
            k.update_weights(d_raw, d_ld, n, w, info)
            got_info = info[:8].cpu().numpy()
            out.append((w.cpu().numpy(), got_info, int(got_info[:1].view(np.int32)[0])))
    finally:
        switch(before)
    return out


def _check(got, cands, fallback, num_valid, num_under, stats, what):
    w, info, best = got
    j = X.match(w, cands)
    if j < 0:   # say how far off before failing
        with np.errstate(all="ignore"):
            c = cands[0]
            bad = np.flatnonzero(~((w == c) | (np.isnan(w) & np.isnan(c))))
            print(f"{what}: {len(bad)} of {len(w)} weights differ from candidate 0 of {len(cands)}; first at {bad[:1]}: "
                  f"{w[bad[:1]]} against {c[bad[:1]]}; NaN written: {int(np.isnan(w).sum())}, in the candidate: "
                  f"{int(np.isnan(c).sum())}")
    assert j >= 0, f"{what}: the weights are none of the {len(cands)} candidates"
    assert X.same(info[1:4], np.asarray(stats, f32)), (what, info[1:4], stats)      # the chains, bit for bit
    assert float(info[4]) == (1.0 if fallback else 0.0), (what, info[4], fallback)
    assert (float(info[5]), float(info[6])) == (float(num_valid), float(num_under)), (what, info[5:7])
    assert best == X.first_max(w), (what, best)              # of the weights as written
    assert best == X.first_max(cands[j]), (what, best)       # and of the candidate they are


@pytest.mark.parametrize("n", X.GPU_SIZES)
@pytest.mark.parametrize("dist", list(X.DISTS))
@pytest.mark.parametrize("kind", list(X.KINDS))
def test_weights_are_a_candidate_on_both_paths(k, kind, dist, n):
    raw, ld, cands, fallback, num_valid, num_under, stats = X.model(kind, dist, n)
    got = _both_paths(k, raw, ld)
    for on, g in zip((1, 0), got):
        _check(g, cands, fallback, num_valid, num_under, stats, f"switch {on}")
    assert got[0][1].tobytes() == got[1][1].tobytes()        # info[:8], byte for byte


def _spread(n):
    """Three indices in three waves of either one-workgroup kernel (thread i % 1024 or i % 512 takes weight i; where the
    size allows, the smallest index in the highest wave) and, above 32 768, in three workgroups of the passes (workgroup
    i // ceil(n / 256)) that sit in three waves of the last pass's tree (workgroup g's candidate goes to thread g)."""
    if n > 32_768:
        per = -(-n // 256)
        return (70 * per + per - 1, 130 * per, 200 * per + per // 2)
    if n > 4096:
        return (1987, 2177, 3399)     # waves 15, 2, 5 of 16; 7, 2, 5 of 8
    if n > 1024:
        return (453, 642, 1024)       # waves 7, 10, 0 of 16; 7, 2, 0 of 8
    return (70, 200, 512)             # waves 1, 3, 8 of 16; 1, 3, 0 of 8


@pytest.mark.parametrize("where", ["last, middle, n // 7", "three waves, three workgroups"])
@pytest.mark.parametrize("n", TIE_SIZES)
def test_argmax_takes_the_first_of_three_equal_maxima(k, where, n):
    idx = (n - 1, n // 2, n // 7) if where.startswith("last") else _spread(n)
    assert len(set(idx)) == 3 and max(idx) < n
    if not where.startswith("last"):
        if n <= 32_768:
            assert all(len({(i % nt) // 64 for i in idx}) == 3 for nt in (1024, 512))
        else:
            assert len({i // -(-n // 256) // 64 for i in idx}) == 3
    raw = X.make_case("three values", "saturated", n)[0].copy()
    raw[list(idx)] = f32(7.0)          # above every other weight; d = 1 keeps equal weights equal and the order of the rest
    ld = X.make_case("three values", "saturated", n)[1]
    cands, fallback, num_valid, num_under, stats = X.candidates(raw, ld)
    got = _both_paths(k, raw, ld)
    for on, g in zip((1, 0), got):
        _check(g, cands, fallback, num_valid, num_under, stats, f"switch {on}")
        w = g[0]
        top = np.flatnonzero(w == w.max())
        assert sorted(top.tolist()) == sorted(idx)           # the maximum at the three indices and nowhere else
        assert g[2] == min(idx), (on, g[2], idx)
    assert got[0][1].tobytes() == got[1][1].tobytes()


@pytest.mark.parametrize("n", TIE_SIZES)
def test_argmax_of_all_equal_weights_is_zero(k, n):
    raw, ld, cands, fallback, num_valid, num_under, stats = X.model("three values", "zero", n)
    for on, g in zip((1, 0), _both_paths(k, raw, ld)):
        _check(g, cands, fallback, num_valid, num_under, stats, f"switch {on}")
        assert len(np.unique(g[0].view(np.uint32))) == 1     # d = 0: every weight the same float
        assert g[2] == 0, (on, g[2])
