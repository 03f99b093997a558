#!/usr/bin/env python3
"""Times the pictures on the GPU: the batched particle picture against a loop of tdr_filter_visualize,
the scan picture against the download it replaces, the label background against the BGR upload.

    python tools/time_pictures.py [--ks 1,4,16,64] [--reps 20] [--out FILE]
    python tools/time_pictures.py --trace-k 16        # one call of each batched picture and its loop, for a kernel trace

Every timed call ends in its own device wait (the entry points return the image on the host), so the host clock around
the call is the call's time.  Medians of `--reps` calls after `--warmup`; the batch / loop comparison is run three times
alternating, and the loop's max - min over the three medians is printed as the margin."""
import argparse
import ctypes as C
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
vp = C.c_void_p
F32 = np.float32


def P(a):
    return a.ctypes.data_as(vp)


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def spread_states(n, H, W, seed):
    from top_down_renderer_amd.batch import STATE_DTYPE
    rng = np.random.default_rng(seed)
    st = np.zeros(n, STATE_DTYPE)
    st["init_x_px"], st["init_y_px"] = W / 2, H / 2
    st["dx_m"], st["dy_m"] = rng.normal(0, 0.05 * W, n), rng.normal(0, 0.05 * H, n)
    st["theta"], st["scale"], st["have_init"] = rng.uniform(-3, 3, n), 1.0, 1
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,4,16,64")
    ap.add_argument("--particles", type=int, default=20000)
    ap.add_argument("--bg", type=int, default=4000)
    ap.add_argument("--pub-scale", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace-k", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import _lib, batch, synth
    from top_down_renderer_amd._lib import VizRequestC, check
    L = _lib.load()
    if L.tdr_device_count() < 1:
        sys.exit("time_pictures: no HIP device (timings are taken on the GPU only)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ks = [a.trace_k] if a.trace_k else [int(k) for k in a.ks.split(",")]
    kmax = max(ks)
    reps, warmup = (1, 1) if a.trace_k else (a.reps, a.warmup)
    sc = synth.make_scene("c1", n_particles=16)
    m = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    m.sample_pts_polar(sc.cfg.nb, sc.cfg.nr, sc.cfg.ang_res)
    H = W = a.bg
    bg = np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)
    params = pkg.FilterParams(fixed_scale=1.0)
    fs = []
    for i in range(kmax):
        f = batch.FilterHandle(m, a.particles, params, seed=100 + i)
        f.set_states(spread_states(a.particles, H, W, i))
        f.set_viz_background(bg)
        fs.append(f)
    oh, ow = int(F32(H) * F32(a.pub_scale)), int(F32(W) * F32(a.pub_scale))
    outs = [np.zeros((oh, ow, 3), np.uint8) for _ in range(kmax)]
    s = C.c_float(a.pub_scale)
    say(f"# particle picture: {a.particles} particles, {H} x {W} background per filter, pub_scale {a.pub_scale} -> {oh} x {ow}; "
        f"medians of {reps} [ms]")
    for k in ks:
        arr = (vp * k)(*[f.h for f in fs[:k]])
        req = (VizRequestC * k)()
        for i in range(k):
            req[i].out_bgr_host, req[i].capacity = outs[i].ctypes.data, outs[i].size
        h_, w_ = C.c_int(), C.c_int()

        def loop():
            for i in range(k):
                check(L.tdr_filter_visualize(fs[i].h, s, None, 0, P(outs[i]), outs[i].size, C.byref(h_), C.byref(w_)))

        def one():
            check(L.tdr_batch_visualize(arr, k, s, req, None))

        loop()
        want = [o.copy() for o in outs[:k]]
        for o in outs[:k]:
            o[...] = 0
        one()
        assert all(np.array_equal(o, w) for o, w in zip(outs[:k], want)), "the batch and the loop draw different pictures"
        tl, tb = [], []
        for _ in range(1 if a.trace_k else 3):
            tl.append(median_ms(loop, reps, warmup))
            tb.append(median_ms(one, reps, warmup))
        say(f"K={k:3d}  loop of K tdr_filter_visualize {statistics.median(tl):9.3f}  tdr_batch_visualize {statistics.median(tb):9.3f}  "
            f"margin (loop max-min of 3) {max(tl) - min(tl):7.3f}  runs loop {['%.3f' % t for t in tl]} batch {['%.3f' % t for t in tb]}")

    # ---- the scan picture ------------------------------------------------------------------------------------------------
    lut = np.random.default_rng(1).integers(0, 256, (256, 3), dtype=np.uint8)
    say(f"# scan picture: medians of {reps} [ms]")
    for nb, nr, ncls in ((100, 25, 6), (256, 256, 6)):
        K = a.trace_k or 16
        unf = np.arange(ncls, dtype=np.int32)
        flat = (np.arange(256) % ncls).astype(np.int32)
        rs = [batch.Renderer(flat) for _ in range(K)]
        rng = np.random.default_rng(2)
        for r in rs:
            pts = np.zeros((20000, 8), F32)
            pts[:, :2] = rng.uniform(-0.5 * nr, 0.5 * nr, (20000, 2))
            pts[:, 4] = rng.integers(0, ncls, 20000)
            r.render_polar(pts, 8, 4, 1.0, 2 * math.pi / nb, ncls, nb, nr)
        img = np.zeros((ncls, nr, nb), F32)
        pic = np.zeros((K, nr, nb, 3), np.uint8)
        h_, w_ = C.c_int(), C.c_int()
        arr = (vp * K)(*[r.h for r in rs])

        def viz1():
            check(L.tdr_renderer_visualize(rs[0].h, P(unf), P(lut), P(pic[0]), pic[0].size, C.byref(h_), C.byref(w_)))

        def get1():
            check(L.tdr_renderer_get_render(rs[0].h, P(img), None))

        def vizK():
            for i in range(K):
                check(L.tdr_renderer_visualize(rs[i].h, P(unf), P(lut), P(pic[i]), pic[i].size, C.byref(h_), C.byref(w_)))

        def getK():
            for i in range(K):
                check(L.tdr_renderer_get_render(rs[i].h, P(img), None))

        def batchK():
            check(L.tdr_batch_scan_pictures(arr, K, P(unf), P(lut), P(pic), None))

        say(f"{nb}x{nr}x{ncls}  tdr_renderer_visualize {median_ms(viz1, reps, warmup):8.4f}  tdr_renderer_get_render (images) "
            f"{median_ms(get1, reps, warmup):8.4f}  |  K={K}: tdr_batch_scan_pictures {median_ms(batchK, reps, warmup):8.4f}  "
            f"K x visualize {median_ms(vizK, reps, warmup):8.4f}  K x get_render {median_ms(getK, reps, warmup):8.4f}")

    # ---- the label background ----------------------------------------------------------------------------------------------
    if not a.trace_k:
        lab = np.random.default_rng(3).integers(0, 256, (H, W), dtype=np.uint8)
        col = lut[lab]
        f = fs[0]
        t_lab = median_ms(lambda: check(L.tdr_filter_set_viz_background_labels(f.h, P(lab), H, W, P(lut))), 5, 1)
        t_bgr = median_ms(lambda: check(L.tdr_filter_set_viz_background(f.h, P(col), H, W)), 5, 1)
        say(f"# label background {H} x {W}, medians of 5 [ms] (wall clock of the call; the old path's host colouring is not timed)")
        say(f"tdr_filter_set_viz_background_labels {t_lab:9.3f}  tdr_filter_set_viz_background {t_bgr:9.3f}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
