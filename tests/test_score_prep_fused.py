"""The scan-side preparation of an integer-form scoring call (csrc/tdr_score_su.hip, tdr_score_ray.hip): the descriptors of
the (direction, ring) bins in the shift-uniform kernel's layout and in the ray-mapped kernel's, the bounding boxes, the list of
bins that hold several classes and the words behind the order's counts (n_list, the `inexact` flags, the mass bound), which
the ordering passes zero and the preparation kernels add to.  The two scoring kernels read one layout each and form exact
integer sums, so scoring every particle through one and then through the other cross-checks everything the preparation
writes: the raw weights are the same BITS.  Run with `pytest -m gpu`.

Shapes (nb, nr): ragged ring groups, a ring count that is no multiple of 64, a direction count that rules the ray-mapped
kernel's patch order out."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_TOTAL = 1_000_000
NCLS = 3
SHAPES = ((32, 24), (40, 22), (64, 70), (100, 25))
ALL_DENSE, ALL_SCATTERED = 0.0, 1e-6   # the span: 0 = every particle counts as dense (tdr_config_shift_uniform_span)


@pytest.fixture(scope="module")
def tdr():
    import torch
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd.kernels import HipKernels

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return pkg, HipKernels()


def _scene(nb, nr):
    """Three classes on a 128 x 128 map that is known everywhere but in one hole; 512 particles of two heading bins within a
    few cells of (64, 64), and 16 spread over the map at headings of their own."""
    from top_down_renderer_amd import synth
    cfg = synth.Config("prep", 4000, NCLS, nb, nr, 128, 528, seed=7100 + nb)
    sc = synth.make_scene(cfg)
    maps = sc.class_maps.copy()
    mask = np.zeros((128, 128), np.uint8)
    mask[78:84, 78:84] = 1
    maps[:, mask == 1] = 0
    rng = np.random.default_rng(nb * 100 + nr)
    st = np.zeros(528, synth.STATE_DTYPE)
    st["scale"] = 1.0
    st["have_init"] = 1
    st["init_x_px"][:512] = rng.normal(64.0, 1.0, 512).clip(60.5, 67.5)
    st["init_y_px"][:512] = rng.normal(64.0, 1.0, 512).clip(60.5, 67.5)
    st["theta"][:200] = 2 * np.pi * 3 / nb
    st["theta"][200:512] = 2 * np.pi * 5 / nb
    gx, gy = np.meshgrid([16.0, 48.0, 80.0, 112.0], [16.0, 48.0, 80.0, 112.0])
    st["init_x_px"][512:] = gx.ravel() + 0.25
    st["init_y_px"][512:] = gy.ravel() + 0.25
    st["theta"][512:] = rng.uniform(-np.pi, np.pi, 16)
    return sc, maps.astype(np.float32), mask, st


class Setup:
    def __init__(self, tdr, oracle, nb, nr):
        import torch
        pkg, k = tdr
        self.k = k
        sc, maps, mask, st = _scene(nb, nr)
        self.cfg = sc.cfg
        self.m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), maps, mask, kernels=k)
        assert self.m.dev.desc.cwords > 0
        self.m.samplePtsPolar((nb, nr), self.cfg.ang_res)
        self.scan = oracle.raster_polar(sc.pts, self.cfg.res, self.cfg.ang_res, sc.lut, NCLS, nb, nr).astype(np.float32)
        self.f = pkg.ParticleFilter(len(st), self.m, pkg.FilterParams(fixed_scale=1.0), kernels=k, init_particles=False,
                                    locality_every=1)
        self.f.set_states(st)
        self.n = len(st)
        self.perm = k.zeros((self.f.cap_local,), torch.int32)
        k.locality_order(self.f.st, self.n, self.m.rows, self.m.cols, self.perm)

    def score(self, scan, mode, span):
        """raw weights, and how many shift-uniform launches the call made"""
        k, f = self.k, self.f
        k.lib.tdr_config_shift_uniform(mode)
        k.lib.tdr_config_shift_uniform_span(span)
        pk = self.m.scan_handle(scan)
        launches = int(k.lib.tdr_shift_uniform_launches())
        f.raw_w.fill_(-7.0)
        k.score(self.m.dev, pk, float(self.cfg.res), f.fp_c, f.st, self.n, f.raw_w, perm=self.perm,
                uniform_scale=f._uniform_scale, n_total=N_TOTAL)
        k.synchronize()
        raw = f.raw_w[:self.n].cpu().numpy()
        assert not (raw == -7.0).any()
        return raw, int(k.lib.tdr_shift_uniform_launches()) - launches


@pytest.fixture(scope="module")
def restore(tdr):
    _, k = tdr
    mode = k.lib.tdr_config_shift_uniform(-1)

    def back():
        k.lib.tdr_config_shift_uniform(mode)
        k.lib.tdr_config_shift_uniform_span(-2.0)
    return back


def _float_agrees(raw_float, raw_int):
    """the float form to its rounding (tests/test_ray.py, tests/test_shift_uniform.py: 3e-6), NaN in the same places"""
    assert np.array_equal(np.isnan(raw_float), np.isnan(raw_int))
    ok = ~np.isnan(raw_int)
    assert ok.any()
    err = np.abs(raw_float[ok] - raw_int[ok]) / np.maximum(np.abs(raw_int[ok]), 1e-30)
    assert err.max() <= 3e-6, err.max()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_both_descriptor_layouts_give_the_same_bits(tdr, oracle, restore, shape):
    """(a) every particle through the shift-uniform kernel == every particle through the ray-mapped kernel, bit for bit;
    (b) both agree with the float form."""
    s = Setup(tdr, oracle, *shape)
    try:
        raw_float, l0 = s.score(s.scan, 0, ALL_DENSE)
        dense, l1 = s.score(s.scan, 2, ALL_DENSE)
        scattered, l2 = s.score(s.scan, 2, ALL_SCATTERED)
    finally:
        restore()
    assert (l0, l1, l2) == (0, 1, 1)
    assert np.isnan(dense).sum() < s.n
    assert np.array_equal(dense, scattered, equal_nan=True)
    _float_agrees(raw_float, dense)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fractional_counts_and_bins_of_several_classes(tdr, oracle, restore, shape):
    """(c) A scan with a fractional count has no integer form: the device raises `inexact`, the integer kernels return and the
    float kernel behind them does the launch — the weights are the BITS of the plain float launch, with every particle dense
    and with every particle scattered.  A bin that holds two classes goes through the packed record (shift-uniform kernel)
    and through the list of multi-class bins (ray-mapped kernel): same bits, the float form to rounding, and the bin counts
    (the weights differ from those of the scan without it).  The fallback before and after an integer launch on the same
    workspace: the words the flags live in are zeroed anew by every call."""
    nb, nr = shape
    s = Setup(tdr, oracle, nb, nr)
    base = s.scan
    occupied = np.flatnonzero(base.sum(axis=0) > 0)
    assert len(occupied) > 4
    frac = base.copy()
    frac[1, occupied[len(occupied) // 2]] += 0.5
    multi = base.copy()
    for b in (occupied[0], occupied[-1], (nr - 1) * nb + nb // 2):   # (the last: the outermost ring, in the ragged ring group)
        multi[0, b] += 2.0
        multi[2, b] += 3.0
    try:
        f_float, _ = s.score(frac, 0, ALL_DENSE)
        f_dense, l1 = s.score(frac, 2, ALL_DENSE)
        base_dense, _ = s.score(base, 2, ALL_DENSE)          # an integer launch between two fallbacks
        f_scattered, l2 = s.score(frac, 2, ALL_SCATTERED)
        m_float, _ = s.score(multi, 0, ALL_DENSE)
        m_dense, _ = s.score(multi, 2, ALL_DENSE)
        m_scattered, _ = s.score(multi, 2, ALL_SCATTERED)
    finally:
        restore()
    assert (l1, l2) == (1, 1)                                # the integer launch was made, found the flag and returned
    assert np.array_equal(f_dense, f_float, equal_nan=True)
    assert np.array_equal(f_scattered, f_float, equal_nan=True)
    assert not np.array_equal(f_float, base_dense, equal_nan=True)
    assert np.array_equal(m_dense, m_scattered, equal_nan=True)
    _float_agrees(m_float, m_dense)
    assert not np.array_equal(m_dense, base_dense, equal_nan=True)
