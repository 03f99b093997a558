"""The particle picture (include/tdr.h, "the particle picture"; csrc/tdr_viz.hip) timed on one MI355X, one process:

  launches       HIP events around each of the three launches (particles, overlay segments, compose) on torch buffers,
                 behind the memset that clears the planes;
  visualize      host clock around the whole tdr_filter_visualize of a C handle, read-back included;
  get_states     host clock around tdr_filter_get_states at the same particle count: the download the host-side
                 visualize(cv::Mat&) cannot avoid, before it draws anything;

per shape (particles on a --image x --image background), cloud (spread: uniform over the image, as after
initializeParticles; converged: sigma = 3 px) and published scale.  Prints one JSON line per cell, times in ms.

--root DIR imports the package from another checkout (a build of the parent commit) and --no-viz then times only
get_states there; --bench also runs that checkout's `bench.py --gpus 1 --config c2 --no-cpu` in a child process.

    python tools/time_viz.py --particles 100000 2000000 --scales 1 0.2 --bench"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np


def summary(ms):
    return {"min": round(min(ms), 4), "median": round(statistics.median(ms), 4), "max": round(max(ms), 4), "n": len(ms)}


def cloud(kind, n, size, dtype):
    rng = np.random.default_rng(11)
    st = np.zeros(n, dtype)
    if kind == "spread":
        st["dx_m"], st["dy_m"] = rng.uniform(0, size, n), rng.uniform(0, size, n)
    else:
        st["dx_m"], st["dy_m"] = rng.normal(size / 2, 3.0, n), rng.normal(size / 2, 3.0, n)
    st["theta"] = rng.uniform(-np.pi, np.pi, n)
    st["scale"], st["have_init"] = 1.0, 1
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--image", type=int, default=4000)
    ap.add_argument("--particles", type=int, nargs="+", default=[100000, 2000000])
    ap.add_argument("--scales", type=float, nargs="+", default=[1.0, 0.2])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-viz", action="store_true", help="time tdr_filter_get_states only (a checkout without the picture)")
    ap.add_argument("--bench", action="store_true", help="also run the checkout's bench.py (config c2, --no-cpu)")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    assert torch.cuda.is_available(), "time_viz needs a HIP device"
    torch.cuda.set_device(0)
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import _lib, synth
    from top_down_renderer_amd._lib import check
    from top_down_renderer_amd.kernels import HipKernels
    k, L = HipKernels(), _lib.load()
    vp = C.c_void_p

    def P(a):
        return a.ctypes.data_as(vp)

    sc = synth.make_scene("c1", n_particles=64)          # any map: the picture reads particle states only
    ncls, mh, mw = sc.class_maps.shape
    m = vp()
    check(L.tdr_map_create(C.byref(m)))
    maps_cm = np.ascontiguousarray(np.transpose(sc.class_maps, (0, 2, 1)), np.float32)
    mask_cm = np.ascontiguousarray(sc.class_mask.T, np.uint8)
    check(L.tdr_map_set(m, P(maps_cm), P(mask_cm), ncls, mh, mw, C.c_float(1.0), 0, 0))
    check(L.tdr_map_sample_pts_polar(m, sc.cfg.nb, sc.cfg.nr, C.c_float(sc.cfg.ang_res)))
    fp = pkg.FilterParams(fixed_scale=1.0).to_c(ncls)
    S = args.image
    bg = np.random.default_rng(1).integers(0, 256, (S, S, 3), dtype=np.uint8)
    sync = torch.cuda.synchronize

    def wall(fn):
        for _ in range(args.warmup):
            fn()
        ms = []
        for _ in range(args.reps):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ms.append((time.perf_counter() - t0) * 1e3)
        return summary(ms)

    for n in args.particles:
        f = vp()
        check(L.tdr_filter_create(m, n, C.byref(fp), 1, C.byref(f)))
        if not args.no_viz:
            check(L.tdr_filter_set_viz_background(f, P(bg), S, S))
            bg_d, planes, dev = k.to_device(bg), k.viz_planes(S, S), k.zeros((7, n))
        for kind in ("spread", "converged"):
            st = cloud(kind, n, S, pkg.STATE_DTYPE)
            check(L.tdr_filter_set_states(f, P(st), n))
            back = np.zeros(n, pkg.STATE_DTYPE)
            row = {"particles": n, "image": S, "cloud": kind,
                   "get_states_wall": wall(lambda: check(L.tdr_filter_get_states(f, P(back), n)))}
            if args.no_viz:
                print(json.dumps(row), flush=True)
                continue
            k.states_to_device(st, dev, n)
            arrows = np.asarray([[S // 2 - 5, S // 2, S // 2 + 5, S // 2]], np.int32)      # the node's ground-truth arrow
            segs = k.to_device(np.asarray([[a[0], a[1], a[2], a[3], 3] for a in arrows.tolist()] * 100, np.int32))  # ~ a mixture's edges
            for s in args.scales:
                oh = ow = int(np.float32(S) * np.float32(s))
                out = k.empty((oh, ow, 3), torch.uint8)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                times = {"particles": [], "segments": [], "compose": []}
                for rep in range(args.warmup + args.reps):
                    planes.zero_()
                    ev[0].record()
                    check(L.tdr_k_viz_particles(dev.data_ptr(), n, n, S, S, planes.data_ptr(), k.stream()))
                    ev[1].record()
                    check(L.tdr_k_viz_segments(segs.data_ptr(), len(segs), S, S, planes.data_ptr(), k.stream()))
                    ev[2].record()
                    check(L.tdr_k_viz_compose(bg_d.data_ptr(), S, S, planes.data_ptr(), oh, ow, out.data_ptr(), k.stream()))
                    ev[3].record()
                    sync()
                    if rep >= args.warmup:
                        for i, name in enumerate(times):
                            times[name].append(ev[i].elapsed_time(ev[i + 1]))
                host = np.zeros((oh, ow, 3), np.uint8)
                h, w = C.c_int(0), C.c_int(0)
                cell = dict(row, pub_scale=s, out=[oh, ow], launches={name: summary(v) for name, v in times.items()},
                            launches_median_sum=round(sum(statistics.median(v) for v in times.values()), 4),
                            visualize_wall=wall(lambda: check(L.tdr_filter_visualize(f, C.c_float(s), P(arrows), 1, P(host),
                                                                                     host.size, C.byref(h), C.byref(w)))))
                print(json.dumps(cell), flush=True)
        L.tdr_filter_destroy(f)
    L.tdr_map_destroy(m)
    if args.bench:
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--config", "c2", "--no-cpu"],
                             capture_output=True, text=True, cwd=root)
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        res = json.loads(line[-1]) if line else {"error": out.stderr[-400:]}
        print(json.dumps({"bench": "c2 --no-cpu", "ms_per_step": res.get("ms_per_step"), "steps": res.get("steps"),
                          "particles_total": res.get("particles_total"), "error": res.get("error")}), flush=True)


if __name__ == "__main__":
    main()
