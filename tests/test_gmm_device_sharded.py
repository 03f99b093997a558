"""tdr_filter_compute_gmm_device on a sharded filter: two ranks over the caller-supplied transport of
tests/test_sharded_handle.py (the collectives are done by this test: device -> host -> gloo -> device).  The samples come
through the all-gather inside the call, every rank runs the same deterministic device fit, and both ranks must store the
same bytes as the plain one-rank filter's device fit."""
import ctypes as C
import os
import socket
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 4096


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _states():
    """Three clusters of particles (sigma 8 / 15 / 5 px, headings within 1 mrad), shuffled."""
    from top_down_renderer_amd import synth
    rng = np.random.default_rng(5)
    st = np.zeros(N, synth.STATE_DTYPE)
    which = rng.integers(0, 3, N)
    cen = np.asarray([(100, 200, 0.3), (400, 250, -2.0), (250, 600, 1.5)])
    sig = np.asarray([8.0, 15.0, 5.0])
    st["init_x_px"] = rng.normal(cen[which, 0], sig[which])
    st["init_y_px"] = rng.normal(cen[which, 1], sig[which])
    st["theta"] = rng.normal(cen[which, 2], 0.001)
    st["scale"], st["have_init"] = 1.0, 1
    return st


def _run(sharded, rank, world, out_path, dist=None):
    import torch
    from top_down_renderer_amd import _lib, synth
    from top_down_renderer_amd._lib import FilterParamsC, check
    L = _lib.load()
    torch.cuda.set_device(0)
    sc = synth.make_scene(synth.Config("gmmshard", 2000, 6, 64, 48, 700, 16, seed=78))
    ncls, H, W = sc.class_maps.shape
    vp = C.c_void_p

    def P(a):
        return a.ctypes.data_as(vp)

    m = vp()
    check(L.tdr_map_create(C.byref(m)))
    maps_cm = np.ascontiguousarray(np.transpose(sc.class_maps, (0, 2, 1)), np.float32)
    mask_cm = np.ascontiguousarray(sc.class_mask.T, np.uint8)
    check(L.tdr_map_set(m, P(maps_cm), P(mask_cm), ncls, H, W, C.c_float(1.0), 0, 0))
    check(L.tdr_map_sample_pts_polar(m, 64, 48, C.c_float(2 * np.pi / 64)))
    fp = FilterParamsC()
    fp.pos_cov, fp.theta_cov, fp.regularization = 0.3, np.pi / 100, 0.15
    fp.init_pos_px_x = fp.init_pos_px_y = fp.init_pos_px_cov = -1
    fp.init_pos_m_x = fp.init_pos_m_y = float("inf")
    fp.init_pos_deg_theta, fp.init_pos_deg_cov = float("inf"), 10
    fp.fixed_scale, fp.scale_log_min, fp.scale_log_max, fp.num_classes = 1.0, -0.1, 1.0, ncls
    for i in range(ncls):
        fp.class_weights[i] = 1.0
    comm, keep, f = vp(), [], vp()
    if sharded:
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
        hip.hipStreamSynchronize.argtypes = [vp]
        AG = C.CFUNCTYPE(C.c_int, vp, vp, vp, C.c_size_t, vp)
        BC = C.CFUNCTYPE(C.c_int, vp, vp, C.c_size_t, C.c_int, vp)

        def all_gather(ctx, send, recv, nbytes, stream):
            hip.hipStreamSynchronize(stream)
            mine = torch.empty(nbytes, dtype=torch.uint8)
            assert hip.hipMemcpy(mine.data_ptr(), send, nbytes, 2) == 0           # device -> host
            parts = [torch.empty(nbytes, dtype=torch.uint8) for _ in range(world)]
            dist.all_gather(parts, mine)
            allb = torch.cat(parts)
            assert hip.hipMemcpy(recv, allb.data_ptr(), nbytes * world, 1) == 0    # host -> device
            return 0

        def broadcast(ctx, buf, nbytes, root, stream):
            hip.hipStreamSynchronize(stream)
            t = torch.empty(nbytes, dtype=torch.uint8)
            if rank == root:
                assert hip.hipMemcpy(t.data_ptr(), buf, nbytes, 2) == 0
            dist.broadcast(t, src=root)
            if rank != root:
                assert hip.hipMemcpy(buf, t.data_ptr(), nbytes, 1) == 0
            return 0

        class Ops(C.Structure):
            _fields_ = [("ctx", vp), ("all_gather", AG), ("broadcast", BC)]
        ops = Ops(None, AG(all_gather), BC(broadcast))
        keep.append(ops)
        check(L.tdr_comm_create(world, rank, C.byref(ops), C.byref(comm)))
        check(L.tdr_filter_create_sharded(m, N, C.byref(fp), 7, comm, C.byref(f)))
    else:
        check(L.tdr_filter_create(m, N, C.byref(fp), 7, C.byref(f)))
    st = _states()
    check(L.tdr_filter_set_states(f, P(st), N))
    log = {}
    for call in range(2):                 # the second call searches around the count the first one chose
        check(L.tdr_filter_compute_gmm_device(f))
        k = C.c_int(-1)
        means, covs = np.zeros((32, 3), np.float32), np.zeros((32, 9), np.float32)
        check(L.tdr_filter_get_gmm(f, 32, C.byref(k), P(means), P(covs)))
        log.update({f"k{call}": np.int64(k.value), f"means{call}": means[: k.value], f"covs{call}": covs[: k.value],
                    f"count{call}": np.int64(L.tdr_filter_adaptive_count(f))})
    L.tdr_filter_destroy(f)
    if sharded:
        L.tdr_comm_destroy(comm)
    np.savez(out_path, **log)


def _worker(rank, world, port, tmp, sharded):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if sharded:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _run(sharded, rank, world, os.path.join(tmp, f"{'shard' if sharded else 'plain'}{rank}.npz"), dist if sharded else None)
    finally:
        if sharded:
            dist.destroy_process_group()


def test_two_ranks_store_the_one_rank_filter_s_device_fit():
    import torch.multiprocessing as mp
    tmp = tempfile.mkdtemp(prefix="tdr_gmm_shard_")
    mp.spawn(_worker, args=(1, _free_port(), tmp, False), nprocs=1, join=True)
    mp.spawn(_worker, args=(2, _free_port(), tmp, True), nprocs=2, join=True)
    load = lambda n: np.load(os.path.join(tmp, n), allow_pickle=False)  # noqa: E731
    plain, r0, r1 = load("plain0.npz"), load("shard0.npz"), load("shard1.npz")
    assert int(plain["k0"]) == 2 and int(plain["k1"]) == 3      # 1 -> 2 -> 3 clusters, one step per call (:276-297)
    for key in plain.files:
        assert plain[key].tobytes() == r0[key].tobytes() == r1[key].tobytes(), key
