#!/usr/bin/env python3
"""Times the fleet picture on the GPU against the K separate pictures it replaces.

    python tools/time_fleet_picture.py [--ks 4,16,64] [--scales 0.25,1.0] [--reps 7] [--out profiles/time_fleet_picture_v1.txt]

  (a) tdr_batch_visualize over K filters, each with its own device copy of the background: K published images
  (b) tdr_batch_visualize_fleet over the same K filters and the one background their map holds: one published image

The two paths alternate in the same run, three rounds of `--reps` calls after `--warmup` each; every call ends in its own
device wait (the entry points return the images on the host), so the host clock around the call is the call's time.
Medians are printed, with the three rounds' medians beside them.  Also recorded: the device bytes held for backgrounds,
and the time to set the background K times (every filter) against once (the map)."""
import argparse
import ctypes as C
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


def cloud(n, H, W, seed, converged):
    """A converged cloud (3 pixels of standard deviation about a random place) or one spread uniformly over the picture."""
    from top_down_renderer_amd.batch import STATE_DTYPE
    rng = np.random.default_rng(seed)
    st = np.zeros(n, STATE_DTYPE)
    if converged:
        cx, cy = rng.uniform(0.1 * W, 0.9 * W), rng.uniform(0.1 * H, 0.9 * H)
        st["dx_m"], st["dy_m"] = rng.normal(cx, 3.0, n), rng.normal(cy, 3.0, n)
        st["theta"] = rng.normal(rng.uniform(-3, 3), 0.1, n)
    else:
        st["dx_m"], st["dy_m"], st["theta"] = rng.uniform(0, W, n), rng.uniform(0, H, n), rng.uniform(-3, 3, n)
    st["scale"], st["have_init"] = 1.0, 1
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="4,16,64")
    ap.add_argument("--scales", default="0.25,1.0")
    ap.add_argument("--particles", type=int, default=20000)
    ap.add_argument("--bg", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import _lib, batch, synth
    from top_down_renderer_amd._lib import VizRequestC, check
    L = _lib.load()
    if L.tdr_device_count() < 1:
        sys.exit("time_fleet_picture: no HIP device (timings are taken on the GPU only)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ks = [int(k) for k in a.ks.split(",")]
    scales = [float(s) for s in a.scales.split(",")]
    kmax = max(ks)
    sc = synth.make_scene("c1", n_particles=16)
    m = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    m.sample_pts_polar(sc.cfg.nb, sc.cfg.nr, sc.cfg.ang_res)
    H = W = a.bg
    bg = np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)
    params = pkg.FilterParams(fixed_scale=1.0)
    fs = []
    for i in range(kmax):
        f = batch.FilterHandle(m, a.particles, params, seed=100 + i)
        f.set_states(cloud(a.particles, H, W, i, converged=i != 1))   # robot 1 is the one spread uniformly
        fs.append(f)
    pal = np.random.default_rng(1).integers(0, 256, (kmax, 3, 3), dtype=np.uint8)
    say(f"# fleet picture: {a.particles} particles per robot in converged clouds (robot 1 spread uniformly), one {H} x {W} "
        f"background; medians of {a.reps} calls [ms], three alternating rounds")

    # ---- the background: K copies against one ----------------------------------------------------------------------------
    mb = bg.nbytes / 1e6
    for k in ks:
        def per_filter():
            for f in fs[:k]:
                check(L.tdr_filter_set_viz_background(f.h, P(bg), H, W))

        def on_map():
            check(L.tdr_map_set_viz_background(m.h, P(bg), H, W))

        t_k, t_1 = median_ms(per_filter, 3, 1), median_ms(on_map, 3, 1)
        say(f"K={k:3d}  background set  (a) K x tdr_filter_set_viz_background {t_k:9.2f}  (b) tdr_map_set_viz_background {t_1:9.2f}"
            f"   device bytes held  (a) {k * mb:8.1f} MB  (b) {mb:6.1f} MB")

    # ---- the pictures -------------------------------------------------------------------------------------------------------
    for scale in scales:
        oh, ow = int(F32(H) * F32(scale)), int(F32(W) * F32(scale))
        s = C.c_float(scale)
        outs = [np.zeros((oh, ow, 3), np.uint8) for _ in range(kmax)]
        one_out = np.zeros((oh, ow, 3), np.uint8)
        say(f"# pub_scale {scale} -> {oh} x {ow}")
        for k in ks:
            arr = (vp * k)(*[f.h for f in fs[:k]])
            req = (VizRequestC * k)()
            for i in range(k):
                req[i].out_bgr_host, req[i].capacity = outs[i].ctypes.data, outs[i].size
            h_, w_ = C.c_int(), C.c_int()

            def separate():
                check(L.tdr_batch_visualize(arr, k, s, req, None))

            def fleet():
                check(L.tdr_batch_visualize_fleet(arr, k, s, P(pal), None, 0, P(one_out), one_out.size, C.byref(h_),
                                                  C.byref(w_), None))

            ta, tb = [], []
            for _ in range(3):
                ta.append(median_ms(separate, a.reps, a.warmup))
                tb.append(median_ms(fleet, a.reps, a.warmup))
            say(f"K={k:3d}  (a) tdr_batch_visualize {statistics.median(ta):9.3f}  (b) tdr_batch_visualize_fleet "
                f"{statistics.median(tb):9.3f}   rounds (a) {['%.3f' % t for t in ta]} (b) {['%.3f' % t for t in tb]}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
