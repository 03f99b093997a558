"""Particle initialisation (tdr_filter_initialize_particles): the serial host loop (tdr_config_tuning("init_device", 0))
against the device chain (csrc/tdr_init.hip) in one process, on the synthetic 4000^2 map, fixed scale, uniform and normal
initial positions.  Wall clock around each call (both paths end synchronised: the host path uploads its states, the device
path waits for its last window); one untimed call first, then --repeats timed calls on the same filter.  Prints one JSON
line per (mode, N) with min / median / max of both and the ratio of the medians.  Per-kernel split: run it under
`rocprofv3 --kernel-trace --stats -- python tools/time_init.py --only device ...`.

    python tools/time_init.py --ns 20000 250000 2000000 --repeats 5"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, nargs="+", default=[20000, 250000, 2000000])
    ap.add_argument("--modes", nargs="+", default=["uniform", "normal"])
    ap.add_argument("--map-size", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=int, default=0, help="init_window_words (0: the default)")
    ap.add_argument("--only", choices=("host", "device"), default=None, help="time one path (kernel traces)")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    from top_down_renderer_amd import _lib, synth
    L = _lib.load()

    def check(rc):
        _lib.check(rc)

    if args.window:
        L.tdr_config_tuning(b"init_window_words", args.window)
    ncls, size = 4, args.map_size
    lab = synth.make_label_image(size, ncls, np.random.default_rng(0)).astype(np.uint8)
    lut = np.ascontiguousarray(synth.make_lut(ncls), np.int32)
    m = C.c_void_p()
    check(L.tdr_map_create(C.byref(m)))
    check(L.tdr_map_set_labels(m, lab.ctypes.data_as(C.c_void_p), size, size, lut.ctypes.data_as(C.c_void_p), 256, ncls,
                               C.c_float(1.0), 0, 0))
    road = float((lab == 1).mean())
    for mode in args.modes:
        fp = _lib.FilterParamsC()
        fp.pos_cov, fp.theta_cov, fp.regularization = 0.3, np.pi / 100, 0.15
        fp.init_pos_px_x = fp.init_pos_px_y = fp.init_pos_px_cov = -1
        if mode == "normal":
            fp.init_pos_px_x, fp.init_pos_px_y, fp.init_pos_px_cov = size / 2, size / 2, size / 8
        fp.init_pos_m_x = fp.init_pos_m_y = float("inf")
        fp.init_pos_deg_theta, fp.init_pos_deg_cov = float("inf"), 10.0
        fp.fixed_scale, fp.scale_log_min, fp.scale_log_max, fp.num_classes = 1.0, -0.1, 1.0, ncls
        for i in range(ncls):
            fp.class_weights[i] = 1.0
        for n in args.ns:
            row = {"mode": mode, "n": n, "map": size, "road_fraction": round(road, 4),
                   "window_words": int(L.tdr_config_tuning(b"init_window_words", -1))}
            for path, dev in (("host", 0), ("device", 1)):
                if args.only and args.only != path:
                    continue
                L.tdr_config_tuning(b"init_device", dev)
                f = C.c_void_p()
                check(L.tdr_filter_create(m, n, C.byref(fp), 12345, C.byref(f)))
                check(L.tdr_filter_initialize_particles(f))   # untimed: the device path's first call moves the generator there
                ts = []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    check(L.tdr_filter_initialize_particles(f))
                    ts.append((time.perf_counter() - t0) * 1e3)
                assert int(L.tdr_filter_num_particles(f)) == n
                L.tdr_filter_destroy(f)
                row[f"{path}_ms"] = [round(min(ts), 3), round(float(np.median(ts)), 3), round(max(ts), 3)]
            if "host_ms" in row and "device_ms" in row:
                row["speedup_median"] = round(row["host_ms"][1] / row["device_ms"][1], 1)
            print(json.dumps(row), flush=True)
    L.tdr_config_tuning(b"init_device", 1)
    L.tdr_map_destroy(m)


if __name__ == "__main__":
    main()
