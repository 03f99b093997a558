"""Cartesian filter (BASELINE config 4's scoring) through the C handle (tdr_filter_create_cart) and through the Python
ParticleFilter, one process, the same map, scan and particles:

  steady state   propagate + update of a filter whose particles all have headings, the two paths ALTERNATING step by step
                 (so both see the same machine), host clock around each step ending in a device synchronise;
  scoring        the scoring launches of the handle's steady-state steps (tdr_profile_enable: HIP events around each);
  first update   the update of a cold-started filter (no particle has a heading: the 40-candidate search runs, then the
                 regular launch), through both paths, next to 41 x the steady-state scoring time;
  chunk sweep    the handle's first update over tdr_config_tuning("cart_init_chunk") values.

Prints one JSON line per section.  Defaults are config 4's shape (512 x 512 window, 8000^2 map, 200 000 particles).

    python tools/time_cart_filter.py --steps 20 --warmup 5 --chunks 1024 4096 16384"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ms):
    return {"min": round(min(ms), 3), "median": round(statistics.median(ms), 3), "max": round(max(ms), 3), "n": len(ms)}


def same_states(a, b):
    return len(a) == len(b) and all(np.array_equal(a[name], b[name]) for name in
                                    ("init_x_px", "init_y_px", "dx_m", "dy_m", "theta", "scale", "have_init"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, nargs=2, default=[512, 512], metavar=("ROWS", "COLS"))
    ap.add_argument("--map-size", type=int, default=8000)
    ap.add_argument("--particles", type=int, default=200000)
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--first-repeats", type=int, default=2)
    ap.add_argument("--chunks", type=int, nargs="*", default=[], help="cart_init_chunk values to sweep (handle, first update)")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_cart_filter needs a HIP device"
    torch.cuda.set_device(0)
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import batch, synth
    from top_down_renderer_amd.kernels import HipKernels
    k = HipKernels()
    rows, cols = args.window
    cfg = synth.Config("cart", args.points, args.classes, rows, cols, args.map_size, args.particles, polar=False, seed=1237)
    sc = synth.make_scene(cfg)
    n = len(sc.states)
    sync = torch.cuda.synchronize

    # the Python path: as bench.py builds config 4
    m = pkg.TopDownMap(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
    m.setWindow(rows, cols)
    r = pkg.ScanRenderer(sc.lut, kernels=k)
    r.set_output_shape(cfg.ncls, rows, cols)
    r.renderSemanticTopDown(sc.pts, cfg.res)
    scan = r.last_scan()
    # the handle path: its own map handle and renderer, the render kept on the device
    mh = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    mh.set_window(rows, cols)
    rh = batch.Renderer(sc.lut)
    rh.render_cart(sc.pts, 4, 3, cfg.res, cfg.ncls, rows, cols)
    params = pkg.FilterParams(fixed_scale=1.0)

    def make(states):
        h = batch.FilterHandle(mh, n, params, seed=1, cart=True)
        h.set_states(states)
        f = pkg.ParticleFilter(n, m, params, seed=1, kernels=k, locality_every=1, init_particles=False)
        f.set_states(states)
        return h, f

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) * 1e3

    def step_h(h):
        h.propagate(1.0, 0.0, 0.01)
        h.update(rh, cfg.res)

    def step_f(f):
        f.propagate((1.0, 0.0), 0.01)
        f.update(scan, None, cfg.res)

    shape = {"window": [rows, cols], "map": args.map_size, "particles": n, "classes": cfg.ncls}
    # ---- steady state, alternating ---------------------------------------------------------------------------------
    h, f = make(sc.states)
    for _ in range(args.warmup):
        step_h(h)
        step_f(f)
    th, tf = [], []
    for _ in range(args.steps):
        th.append(timed(lambda: step_h(h)))
        tf.append(timed(lambda: step_f(f)))
    same = same_states(h.states(), f.get_states())
    print(json.dumps({"section": "steady_state_step_ms", **shape, "handle": summary(th), "python": summary(tf),
                      "states_identical_after": same}), flush=True)
    # ---- the scoring launches of the handle's steps ----------------------------------------------------------------
    k.lib.tdr_profile_enable(1)
    ms, launches = C.c_double(0), C.c_int64(0)
    k.lib.tdr_profile_score_ms(C.byref(ms), C.byref(launches))
    for _ in range(max(3, args.steps // 4)):
        step_h(h)
    sync()
    k.lib.tdr_profile_score_ms(C.byref(ms), C.byref(launches))
    k.lib.tdr_profile_enable(0)
    score_ms = ms.value / max(launches.value, 1)
    print(json.dumps({"section": "steady_state_scoring_ms", **shape, "per_launch": round(score_ms, 3),
                      "launches": launches.value}), flush=True)
    del h, f
    # ---- first update: cold start ----------------------------------------------------------------------------------
    cold = sc.states.copy()
    cold["have_init"] = 0
    cold["theta"] = 0

    def first_update(chunk=None):
        if chunk is not None:
            k.tuning("cart_init_chunk", chunk)
        h, f = make(cold)
        t_h = timed(lambda: h.update(rh, cfg.res))
        t_f = timed(lambda: f.update(scan, None, cfg.res))
        same = same_states(h.states(), f.get_states())
        return t_h, t_f, same

    default_chunk = k.tuning("cart_init_chunk")
    first_update()   # untimed: allocates the search's workspace sizes, loads every kernel of the path
    res = [first_update() for _ in range(args.first_repeats)]
    print(json.dumps({"section": "first_update_ms", **shape, "cart_init_chunk": default_chunk,
                      "handle": summary([x[0] for x in res]), "python": summary([x[1] for x in res]),
                      "states_identical_after": all(x[2] for x in res),
                      "41_x_steady_state_scoring": round(41 * score_ms, 3)}), flush=True)
    # ---- where the first update's time goes: its scoring launches, and the regular launch over the same cold cloud -----
    # (the steady-state cloud has been resampled onto the pose; the cold one still holds its scattered particles, each of
    # which costs the scattered kernel a whole wave: 41 x ITS regular launch is what the composed search is built from)
    h = batch.FilterHandle(mh, n, params, seed=1, cart=True)
    h.set_states(cold)
    k.lib.tdr_profile_enable(1)
    k.lib.tdr_profile_score_ms(C.byref(ms), C.byref(launches))
    wall = timed(lambda: h.compute_weights(rh, cfg.res))          # the search and the regular launch
    k.lib.tdr_profile_score_ms(C.byref(ms), C.byref(launches))
    search_ms, search_launches = ms.value, launches.value
    again = [timed(lambda: h.compute_weights(rh, cfg.res)) for _ in range(3)]   # every particle has its heading now
    k.lib.tdr_profile_score_ms(C.byref(ms), C.byref(launches))
    k.lib.tdr_profile_enable(0)
    cold_ms = ms.value / max(launches.value, 1)
    print(json.dumps({"section": "first_update_breakdown_ms", **shape, "cart_init_chunk": default_chunk,
                      "compute_weights_with_search_wall": round(wall, 3), "its_scoring_launches": search_launches,
                      "its_scoring_launches_sum": round(search_ms, 3),
                      "outside_the_scoring_launches": round(wall - search_ms, 3),
                      "regular_launch_on_the_cold_cloud": round(cold_ms, 3),
                      "41_x_regular_launch_on_the_cold_cloud": round(41 * cold_ms, 3),
                      "compute_weights_without_search_wall": summary(again)}), flush=True)
    del h
    for chunk in args.chunks:
        first_update(chunk)
        res = [first_update(chunk) for _ in range(args.first_repeats)]
        print(json.dumps({"section": "first_update_chunk_sweep_ms", **shape, "cart_init_chunk": chunk,
                          "handle": summary([x[0] for x in res]), "python": summary([x[1] for x in res])}), flush=True)
    k.tuning("cart_init_chunk", default_chunk)


if __name__ == "__main__":
    main()
