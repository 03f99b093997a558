"""The scan-side preparation of an integer-form scoring call as ONE kernel (csrc/tdr_score_su.hip: score_prep_kernel, through
tdr_k_score_prep) and the bounded float fallback behind the integer kernels (csrc/tdr_score.hip: score_polar_bounded_kernel,
score_finalize_bounded_kernel).

1. every product of the preparation against a NumPy model written here, element for element;
2. scoring: the same bits whichever kernel scores a particle, with and without the table's factors, on both ordering paths,
   <= 3e-7 relative against the oracle's weights, and nothing survives a call on a workspace;
3. the bounded fallback gives the bits of the plain float launch, also when every workgroup of its grid iterates.

The shapes (nb, nr) and the scene are those of tests/test_score_prep_fused.py: ragged ring groups, ring counts that are no
multiple of 4 and none of 64, direction counts with and without the patch order, sectors of 12.5 directions.
Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

from test_score_prep_fused import ALL_DENSE, ALL_SCATTERED, N_TOTAL, NCLS, SHAPES, Setup, _scene, restore, tdr  # noqa: F401

pytestmark = pytest.mark.gpu

FMAX = np.float32(3.402823466e+38)
CODE_FULL, CODE_PAD = 0xFF, 0xFD


def _several_classes(scan, nb, nr):
    """the scan with three bins of two classes (the outermost ring among them) and one count beyond 12 bits"""
    occupied = np.flatnonzero(scan.sum(axis=0) > 0)
    out = scan.copy()
    for b in (occupied[0], occupied[-1], (nr - 1) * nb + nb // 2):
        out[0, b] += 2.0
        out[2, b] += 3.0
    single = [b for b in occupied[1:-1] if (out[:, b] != 0).sum() == 1][0]
    out[int(np.flatnonzero(out[:, single])[0]), single] = 5000.0
    return out


def _model(lib, m, tab, scan, lay, uscale, res, fac):
    """What score_prep_kernel writes, from the table [nr * nb][2] (entry j * nb + i), the scan [ncls][nr * nb] of whole counts,
    the layout words of tdr_k_score_prep and the factors in the context (None: none)."""
    nb, nr, ncls = m.nb, m.nr, m.ncls
    G, C, _, gq, blocks, bm, patch, T, nbins, S = lay[:10]
    out = {}
    T32 = tab.astype(np.float32)
    if uscale > 0:
        T32 = ((T32 * np.float32(uscale)).astype(np.float32) * np.float32(res)).astype(np.float32)
        out["utab"] = T32
    nz = (scan != 0).sum(axis=0)
    first = np.argmax(scan != 0, axis=0)
    total = scan.sum(axis=0, dtype=np.float64).astype(np.float32)
    vfirst = scan[first, np.arange(nb * nr)]
    rows, cols, cw = m.desc.rows, m.desc.cols, m.desc.cwords
    lc = 3 if cw == 1 else (2 if cw == 2 else 1)
    ckconst = ((rows >> lc) + 2) * 128 + 128
    plane_bytes = int(lib.tdr_cmap_plane_words(ncls, rows, cols)) * 4
    pbase = int(lib.tdr_cmap_plane_offset_words(ncls, rows, cols)) * 4 + ((rows >> 3) + 2) * 128 + 128
    # ---- the shift-uniform layout
    tab_su = np.zeros((C, nb, G, 2), np.float32)
    desc = np.zeros((C, nb, G, 4), np.uint32)
    for c in range(C):
        for jj in range(G):
            j = c * G + jj
            ks = min(j, nr - 1) * nb + np.arange(nb)
            tab_su[c, :, jj] = T32[ks]
            if j >= nr:
                desc[c, :, jj, 0], desc[c, :, jj, 2] = CODE_PAD, ckconst
                continue
            one, many = nz[ks] == 1, nz[ks] > 1
            desc[c, :, jj, 0] = np.where(one, first[ks] + 1, np.where(many, CODE_FULL, 0))
            desc[c, :, jj, 1] = np.where(one, vfirst[ks], np.where(many, total[ks], 0)).astype(np.uint32)
            desc[c, :, jj, 2] = np.where(one, pbase + first[ks] * plane_bytes, ckconst)
    full = (desc[..., 0] >= 0xFE).reshape(C, nb, G // 4, 4).any(axis=3)
    desc[:, :, ::4, 3] = np.where(full, 0x80000000, 0)
    out["tab_su"], out["desc"] = tab_su.reshape(-1, 2), desc.reshape(-1, 4)
    bbox = np.zeros((C, S, 4), np.float32)
    for c in range(C):
        gn = min(nr - c * G, G)
        for s in range(S):
            e = tab_su[c, s * nb // S:(s + 1) * nb // S, :gn].reshape(-1, 2)
            bbox[c, s] = (e[:, 0].min(), e[:, 0].max(), e[:, 1].min(), e[:, 1].max()) if len(e) else (FMAX, -FMAX, FMAX, -FMAX)
    out["bbox"] = bbox
    # ---- the ray-mapped layouts
    rp = blocks * gq * 64
    I, J = np.meshgrid(np.arange(nb), np.arange(rp), indexing="ij")
    real = J < nr
    K = np.minimum(J, nr - 1) * nb + I
    g, l = J >> 6, J & 63
    b = g // gq
    at = np.where(bm, (b * nb + I) * 64 + l, ((I * blocks + b) * 64 + l) * gq + (g - b * gq))
    at_d = at
    if patch:
        at_d = ((((J // 16) * (nb // 16) + I // 16) * 64 + (I & 3) * 16 + (J % 16)) << 2) + ((I % 16) >> 2)
    assert len(np.unique(at)) == at.size and len(np.unique(at_d)) == at.size and at.max() < T and at_d.max() < T
    tab_ray = np.where(real[..., None], T32[K], np.float32(-1.0e30)).astype(np.float32)
    loop = real & (nz[K] == 1) & (vfirst[K] < 4096)
    d = np.where(loop, vfirst[K].astype(np.uint32) | ((first[K] + 1).astype(np.uint32) << 12), 0).astype(np.uint32)
    own = (d >> 12).reshape(nb, rp // 4, 4)
    borrowed = own.copy()
    for ql in range(4):   # an empty bin: the class of the nearest non-empty bin of its four, the lower one where two tie
        for dist in (3, 2, 1):
            for q in (ql + dist, ql - dist):
                if 0 <= q < 4:
                    take = (own[..., ql] == 0) & (own[..., q] != 0)
                    borrowed[..., ql] = np.where(take, own[..., q], borrowed[..., ql])
    d = np.where(d >> 12 != 0, d, borrowed.reshape(nb, rp) << 12).astype(np.uint32)
    out["ray_index"], out["ray_desc_index"] = at.ravel(), at_d.ravel()
    out["tab_ray"], out["desc_ray"] = tab_ray.reshape(-1, 2), d.ravel().astype(np.uint16)
    if fac is not None:
        rad_at = ((b * 64 + l) * gq + (g - b * gq))[0]
        out["rad_index"] = rad_at
        out["rad_ray"] = np.where(real[0], fac[2 * nb + np.minimum(J[0], nr - 1)], np.float32(1.0e30)).astype(np.float32)
        fx = (fac[2 * I] * fac[2 * nb + np.minimum(J, nr - 1)]).astype(np.float32)
        fy = (fac[2 * I + 1] * fac[2 * nb + np.minimum(J, nr - 1)]).astype(np.float32)
        if uscale > 0:
            fx = ((fx * np.float32(uscale)).astype(np.float32) * np.float32(res)).astype(np.float32)
            fy = ((fy * np.float32(uscale)).astype(np.float32) * np.float32(res)).astype(np.float32)
        same = (fx.view(np.uint32) == T32[K][..., 0].view(np.uint32)) & (fy.view(np.uint32) == T32[K][..., 1].view(np.uint32))
        out["not_factors"] = int((~same & real).any())
    else:
        out["not_factors"] = 0
    listed = real & ~loop & (nz[K] >= 1)
    out["list"] = np.sort(((I[listed].astype(np.uint32) << 16) | J[listed].astype(np.uint32)))
    tk = total[(np.arange(nr)[:, None] * nb + np.arange(nb)[None, :]).ravel()]
    # the mass bound: the word holds the sum modulo 2^32 (one bin adds at most 65 536: 65 536 such bins make it 0 again), and the
    # addition that carries the sum to 2^24 or past it raises inexact[0] — a bound of 2^24 or more never passes for a low one
    mass = int(((tk[(tk >= 1) & (tk < 16777216)].astype(np.int64) >> 8) + 1).sum())
    out["mass"], out["mass_off"] = mass & 0xFFFFFFFF, int(mass >= (1 << 24))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_product_against_a_model(tdr, oracle, restore, shape):
    """tab_su, the descriptors (codes, counts, plane constants, the step's "several classes" bit), desc_ray in each order with
    the borrowed classes, tab_ray, rad_ray, the sorted list, n_list, the `inexact` words, the mass bound, utab and the boxes
    (==) — with and without a uniform scale, with and without the table's factors in the context, and with the factors of
    ANOTHER table, where inexact[2] rises and nothing else moves."""
    import torch
    pkg, k = tdr
    nb, nr = shape
    s = Setup(tdr, oracle, nb, nr)
    scan = _several_classes(s.scan, nb, nr)
    dev = s.m.dev
    tab = dev.tab.cpu().numpy().reshape(-1, 2)
    fac_own = dev.fac
    other = np.empty(2 * nb + nr, np.float32)
    assert k.lib.tdr_polar_factors_host(nb, nr, C.c_float(np.float32(s.cfg.ang_res) * np.float32(1.25)),
                                        C.c_float(1.0), other.ctypes.data_as(C.c_void_p)) == 0
    ctx = k.score_ctx_create()
    seen_orders = set()
    try:
        k.lib.tdr_config_shift_uniform(2)
        pk = s.m.scan_handle(scan)
        for uscale in (0.0, 1.0, 0.75):
            for facs in ("none", "own", "other"):
                dev.fac = fac_own if facs != "other" else k.to_device(other)
                lay, got = k.score_prep(dev, pk, float(s.cfg.res), s.f.st, s.n, perm=s.perm, uniform_scale=uscale,
                                        n_total=N_TOTAL, ctx=None if facs == "none" else ctx, span=4.0)
                k.synchronize()
                got = {name: t.cpu().numpy() for name, t in got.items()}
                fac = None if facs == "none" else dev.fac.cpu().numpy()
                want = _model(k.lib, dev, tab, scan, lay, uscale, float(s.cfg.res), fac)
                seen_orders.add((lay[3], lay[5], lay[6]))
                assert lay[0] % 4 == 0 and lay[2] % 64 == 0 and lay[2] >= max(lay[0] * lay[1], lay[3] * lay[4] * 64)
                assert lay[5] == (facs != "none")
                if uscale > 0:
                    assert np.array_equal(got["utab"].view(np.uint32), want["utab"].view(np.uint32))
                assert np.array_equal(got["tab_su"].view(np.uint32), want["tab_su"].view(np.uint32))
                assert np.array_equal(got["desc"].view(np.uint32), want["desc"])
                assert (got["bbox"] == want["bbox"]).all()
                assert np.array_equal(got["tab_ray"].view(np.uint32)[want["ray_index"]], want["tab_ray"].view(np.uint32))
                assert np.array_equal(got["desc_ray"].view(np.uint16)[want["ray_desc_index"]], want["desc_ray"])
                if fac is not None:
                    assert np.array_equal(got["rad_ray"][want["rad_index"]], want["rad_ray"])
                tail = got["tail"]
                assert tail[2] == tail[0] + tail[1] and tail[0] % 64 == 0 and 0 < tail[2] and tail[1] <= s.n
                assert tail[3] == len(want["list"]) and tail[3] >= 3
                assert np.array_equal(np.sort(got["list"][:tail[3]].view(np.uint32)), want["list"])
                assert tail[4] == want["mass_off"] == 0 and tail[5] == want["mass"] and want["mass"] < (1 << 24)
                assert tail[6] == want["not_factors"] == (1 if facs == "other" else 0)
    finally:
        dev.fac = fac_own
        k.lib.tdr_score_ctx_set_polar_factors(ctx.handle, None, 0, 0)
        restore()
    assert (1, 1, 1 if nb % 16 == 0 else 0) in seen_orders and any(o[1] == 0 for o in seen_orders)


@pytest.mark.parametrize("shape,full,extra,bound", (((32, 24), 255, 65534 * 256, (1 << 24) - 1), ((32, 24), 256, 0, 1 << 24),
                                                    ((32, 24), 256, 1, (1 << 24) + 1), ((256, 256), 65536, 0, 1 << 32)),
                         ids=("2p24_minus_1", "2p24", "2p24_plus_1", "2p32_wraps"))
def test_the_mass_bound_and_its_flag_against_the_model(tdr, oracle, restore, shape, full, extra, bound):
    """Bins of 2^24 - 1 add 65 536 each to the bound: below 2^24 the word is the bound and inexact[0] stays down; from 2^24 on
    inexact[0] is up, also where the word itself has wrapped to 0 (65 536 such bins) — int_form_off never sees a low bound."""
    pkg, k = tdr
    nb, nr = shape
    s = Setup(tdr, oracle, nb, nr)
    bins = np.random.default_rng(8).permutation(nb * nr)
    scan = np.zeros_like(s.scan)
    scan[0, bins[:full]] = (1 << 24) - 1
    if extra:
        scan[1, bins[full]] = extra
    try:
        k.lib.tdr_config_shift_uniform(2)
        lay, got = k.score_prep(s.m.dev, s.m.scan_handle(scan), float(s.cfg.res), s.f.st, s.n, perm=s.perm, uniform_scale=0.0,
                                n_total=N_TOTAL, ctx=None, span=4.0)
        k.synchronize()
        tail = got["tail"].cpu().numpy()
        want = _model(k.lib, s.m.dev, s.m.dev.tab.cpu().numpy().reshape(-1, 2), scan, lay, 0.0, float(s.cfg.res), None)
        assert want["mass"] == bound & 0xFFFFFFFF and want["mass_off"] == int(bound >= 1 << 24)
        assert int(tail[5]) & 0xFFFFFFFF == want["mass"] and tail[4] == want["mass_off"]
        assert tail[3] == len(want["list"]) == full + (1 if extra >= 4096 else 0)   # (a single class below 4096: the descriptor)
    finally:
        restore()


def _oracle_weights(oracle, s, scan, ang_res=None):
    _, maps, mask, st = _scene(s.cfg.nb, s.cfg.nr)
    tab = oracle.polar_table(s.cfg.nb, s.cfg.nr, s.cfg.ang_res if ang_res is None else ang_res)
    return oracle.compute_weights(oracle.OracleMap(maps, mask, 1.0), tab, s.cfg.nb, s.cfg.nr, scan, s.cfg.res,
                                  oracle.make_params(NCLS, fixed_scale=1.0), st.copy())


def _close(raw, ref, bound=3e-7):
    assert np.array_equal(np.isnan(raw), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert ok.any()
    err = float(np.max(np.abs(raw[ok].astype(np.float64) - ref[ok]) / np.abs(ref[ok])))
    print(f"max relative difference to the oracle {err:.3e}")
    assert err <= bound, err


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_scoring_gives_the_same_bits_every_way(tdr, oracle, restore, shape):
    """All dense, all scattered, mixed; with and without a context's factors; bucket sort and rocPRIM's order: one set of bits,
    <= 3e-7 relative to the oracle's weights.  A second call on the same workspace with another scan and another table gives
    what a workspace of other contents gives: nothing survives a call."""
    import torch
    pkg, k = tdr
    nb, nr = shape
    s = Setup(tdr, oracle, nb, nr)
    scan = _several_classes(s.scan, nb, nr)
    ctx = k.score_ctx_create()
    bucket = k.tuning("su_order_bucket")

    def score(sc, span, c):
        k.lib.tdr_config_shift_uniform(2)
        k.lib.tdr_config_shift_uniform_span(span)
        s.f.raw_w.fill_(-7.0)
        k.score(s.m.dev, s.m.scan_handle(sc), float(s.cfg.res), s.f.fp_c, s.f.st, s.n, s.f.raw_w, perm=s.perm,
                uniform_scale=s.f._uniform_scale, n_total=N_TOTAL, ctx=c)
        k.synchronize()
        raw = s.f.raw_w[:s.n].cpu().numpy()
        assert not (raw == -7.0).any()
        return raw

    try:
        got = []
        for order in (1, 0):
            k.tuning("su_order_bucket", order)
            for c in (None, ctx):
                for span in (ALL_DENSE, ALL_SCATTERED, 4.0):
                    got.append(score(scan, span, c))
        for g in got[1:]:
            assert np.array_equal(g, got[0], equal_nan=True)
        _close(got[0], _oracle_weights(oracle, s, scan))
        # another scan and another table on the workspace the calls above used, then on one of other contents
        k.tuning("su_order_bucket", bucket)
        ang2 = float(np.float32(s.cfg.ang_res) * np.float32(0.5))
        s.m.samplePtsPolar((nb, nr), ang2)
        scan2 = np.roll(s.scan, 3, axis=1)
        for c in (None, ctx):
            used = score(scan2, 4.0, c)
            k._ws = torch.full_like(k._ws, float("nan"))
            fresh = score(scan2, 4.0, c)
            assert np.array_equal(used, fresh, equal_nan=True)
        _close(used, _oracle_weights(oracle, s, scan2, ang2))
    finally:
        k.tuning("su_order_bucket", bucket)
        k.lib.tdr_score_ctx_set_polar_factors(ctx.handle, None, 0, 0)
        restore()


@pytest.mark.parametrize("waves", (8, 0), ids=("two_workgroups", "default"))
def test_the_bounded_fallback_gives_the_plain_float_launch(tdr, oracle, restore, waves):
    """A fractional count, and a dictionary without an integer form: the float form behind the integer kernels runs on a bounded
    grid — with score_waves = 8 two workgroups, each of which walks many workgroup ids — and gives the BITS of the plain float
    launch (tdr_config_shift_uniform(0)), NaN in the same places."""
    pkg, k = tdr
    nb, nr = 64, 70
    before = k.tuning("score_waves")
    try:
        s = Setup(tdr, oracle, nb, nr)
        frac = s.scan.copy()
        occupied = np.flatnonzero(frac.sum(axis=0) > 0)
        frac[1, occupied[len(occupied) // 2]] += 0.5
        plain, _ = s.score(frac, 0, ALL_DENSE)
        if waves:
            k.tuning("score_waves", waves)
        for span in (ALL_DENSE, ALL_SCATTERED):
            bounded, launches = s.score(frac, 2, span)
            assert launches == 1
            assert np.array_equal(np.isnan(bounded), np.isnan(plain))
            assert np.array_equal(bounded, plain, equal_nan=True)
        k.tuning("score_waves", before)
        # a map that also holds 1e-6: its dictionary has no integer form (tests/test_ray.py)
        _, maps, mask, st = _scene(nb, nr)
        maps[1, 40:60, 50:80] = np.float32(1e-6)
        m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), maps, mask, kernels=k)
        assert m.dev.desc.cwords > 0 and int(m.dev.dict.cpu().numpy()[2049:2050].view(np.uint32)[0]) == 0
        m.samplePtsPolar((nb, nr), s.cfg.ang_res)
        s.m = m
        plain, _ = s.score(s.scan, 0, ALL_DENSE)
        if waves:
            k.tuning("score_waves", waves)
        bounded, launches = s.score(s.scan, 2, 4.0)
        assert launches == 1
        assert np.array_equal(np.isnan(bounded), np.isnan(plain))
        assert np.array_equal(bounded, plain, equal_nan=True)
    finally:
        k.tuning("score_waves", before)
        restore()
