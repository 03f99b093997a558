"""tdr_k_resample_gather (csrc/tdr_filter.hip): running maximum -> resample indices -> gathered state rows, and the
max-likelihood particle of the set BEFORE the resample, in one launch.  Checked against the oracle's resample of the same
weights plus NumPy indexing, and against the three entries it replaces in the unsharded update (tdr_k_resample /
tdr_k_resample_dev, tdr_k_gather_states, tdr_k_save_ml_state), in both source layouts, for a shard's range of the new set,
with the shift as a host value and in device memory."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

f32 = np.float32
N = 300          # old set: more than one block of 256 threads
WORLD, SHARD = 3, 100   # the all-gathered layout of the same 300 particles: [rank][7][100]
CAP = 320        # row length of the plain [7][cap] planes (> N)
SHIFT = 0.37


@pytest.fixture(scope="module")
def k():
    import torch
    from top_down_renderer_amd.kernels import HipKernels

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return HipKernels()


@pytest.fixture(scope="module")
def old_set():
    """(weights, running maximum, state rows [7][N], argmax): a normalised weight vector with zeros and a few dominant
    particles, NumPy's serial float32 running sum (particle_filter.cpp:179) and its running maximum."""
    rng = np.random.default_rng(3300)
    w = rng.random(N).astype(f32) ** 4
    w[rng.random(N) < 0.1] = 0.0
    w[[17, 260]] *= f32(30.0)
    w = (w / w.sum(dtype=np.float64)).astype(f32)
    run = np.cumsum(w, dtype=f32)
    runmax = np.maximum.accumulate(run).astype(f32)
    st = rng.normal(0, 50, (7, N)).astype(f32)
    st[5] = rng.random(N).astype(f32) + f32(0.5)
    st[6] = (rng.random(N) < 0.8).astype(f32)
    return w, runmax, st, 260 if w[260] > w[17] else 17


def _layouts(k, st):
    """{name: (device source, src_shard)}: the plain planes [7][CAP] and the all-gathered [rank][7][SHARD] buffer"""
    plain = np.full((7, CAP), -9.0, f32)
    plain[:, :N] = st
    gathered = np.ascontiguousarray(st.reshape(7, WORLD, SHARD).transpose(1, 0, 2)).reshape(-1)
    return {"planes": (k.to_device(plain), 0), "gathered": (k.to_device(gathered), SHARD)}


def _ml_record(st, best):
    f = st[:, best]
    return np.array([*f, 0.0, f[2] * f[5] + f[0], f[3] * f[5] + f[1], f[4], f[5]], f32)


@pytest.mark.parametrize("layout", ["planes", "gathered"])
@pytest.mark.parametrize("n_new,i_begin,i_end", [(257, 0, 257), (300, 0, 300), (1000, 0, 1000), (1000, 500, 750),
                                                  (300, 257, 300)])
def test_fused_equals_oracle_and_the_three_entries(k, oracle, old_set, layout, n_new, i_begin, i_end):
    import torch
    w, runmax, st, best = old_set
    nl = i_end - i_begin
    src, shard = _layouts(k, st)[layout]
    rm = k.to_device(runmax)
    word = np.zeros(8, np.int32)
    word[0] = best
    info = k.to_device(word.view(f32))   # info[0]: the argmax, as int bits
    idx_ref = oracle.resample_prefix(w, n_new, SHIFT)[i_begin:i_end]
    assert idx_ref.min() >= 0 and idx_ref.max() < N and len(np.unique(idx_ref)) > 3

    # the three separate entries
    idx3 = torch.full((nl + 8,), -5, dtype=torch.int32, device=k.device)
    dst3 = torch.full((7, nl + 8), -5.0, device=k.device)
    ml3 = torch.full((12,), -5.0, device=k.device)
    k.resample(rm, N, n_new, SHIFT, i_begin, i_end, idx3)
    k.gather_states(src, idx3, nl, dst3, src_shard=shard)
    k.save_ml_state(info, src, N, ml3, src_shard=shard)

    from top_down_renderer_amd.kernels import DevPtr
    word_dev = k.to_device(np.array([SHIFT], f32))
    for shift in (SHIFT, word_dev, DevPtr(word_dev.data_ptr())):   # host value / device word / a generator pipe's pointer
        idx = torch.full((nl + 8,), -5, dtype=torch.int32, device=k.device)
        dst = torch.full((7, nl + 8), -5.0, device=k.device)
        ml = torch.full((12,), -5.0, device=k.device)
        k.resample_gather(rm, N, n_new, shift, i_begin, i_end, idx, src, dst, info, ml, src_shard=shard)
        k.synchronize()
        got_idx, got_dst, got_ml = idx.cpu().numpy(), dst.cpu().numpy(), ml.cpu().numpy()
        # the oracle's indices, NumPy's gather, the max-likelihood record of the OLD set
        assert np.array_equal(got_idx[:nl], idx_ref)
        assert np.array_equal(got_dst[:, :nl], st[:, idx_ref])
        assert np.array_equal(got_ml, _ml_record(st, best))
        # nothing written past the range
        assert (got_idx[nl:] == -5).all() and (got_dst[:, nl:] == -5.0).all()
        # and the three entries, byte for byte
        assert np.array_equal(got_idx, idx3.cpu().numpy())
        assert np.array_equal(got_dst, dst3.cpu().numpy())
        assert np.array_equal(got_ml, ml3.cpu().numpy())


def test_filter_update_takes_the_fused_entry_and_keeps_its_results(k, oracle):
    """ParticleFilter.update (unsharded) ends in the one launch: after an update, resample_indices(), the states and
    maxLikelihood() are the oracle's resample of the filter's own weights, NumPy's gather of the pre-resample states and
    that set's argmax particle."""
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import synth
    sc = synth.make_scene("c1", n_particles=N)
    cfg = sc.cfg
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    r = pkg.ScanRendererPolar(sc.lut, kernels=k)
    r.set_output_shape(cfg.ncls, cfg.nb, cfg.nr)
    f = pkg.ParticleFilter(N, m, pkg.FilterParams(fixed_scale=1.0), seed=5, kernels=k, init_particles=False)
    f.set_states(sc.states)
    f.propagate((1.0, 0.0), 0.01)
    r.renderSemanticTopDown(sc.pts, cfg.res, cfg.ang_res)
    before = f.st[:, :N].cpu().numpy().copy()
    f.update(r.last_scan(), None, cfg.res, shift=SHIFT, n_target=257)
    w = f.weights()
    idx_ref = oracle.resample_prefix(w, 257, SHIFT)
    assert f.numParticles() == 257
    assert np.array_equal(f.resample_indices(), idx_ref)
    assert np.array_equal(f.st[:, :257].cpu().numpy(), before[:, idx_ref])
    best = int(np.argmax(w))
    assert np.array_equal(f._ml_buf.cpu().numpy(), _ml_record(before, best))
