"""Start / end time of every workgroup of the two integer-form scoring kernels in ONE scoring call of a bench config, on the
particle set bench.py's timed steps start from: how many workgroups are resident over time, how long one lives, and the IDLE
AREA of the run-down — from the moment the last workgroup is dispatched nothing refills a compute unit, and the chip runs from
full to empty.  Successor of diag_score_timeline.py (the float kernel).

Needs a diagnostic build of the library (every workgroup's thread 0 stamps wall_clock64 at its start and end; the normal
build has none of it), in a directory of its own so that the product's objects stay what they are:

    python tools/su_timeline.py --build DIR          # hipcc -DTDR_SCORE_TIMELINE -> DIR/libtdr_hip_tl.so (no GPU needed)
    TDR_LIB_PATH=DIR/libtdr_hip_tl.so python tools/su_timeline.py [--config c2] [--tail K,Q]      (on the GPU)

"ms at full rate" prices the idle area with DESIGN.md 5.1's occupancy sweep of the dense kernel (6 / 5 / 4 / 3 / 2 waves per
SIMD: 2.83 / 2.96 / 3.28 / 3.92 / 5.53 ms, i.e. relative throughput 1 / 0.96 / 0.86 / 0.72 / 0.51; one wave: half of two, a
guess; none: 0): the time the run-down takes minus the time its work would take with the chip full."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TL_MAX = 1 << 17                     # TDR_TL_MAX (csrc/tdr_score_dev.h)
RATE = np.array([0.0, 0.255, 0.51, 0.72, 0.86, 0.96, 1.0])   # relative throughput at 0..6 sixths of the resident capacity


def build(out_dir):
    from top_down_renderer_amd import build as b
    os.makedirs(out_dir, exist_ok=True)
    b.OUT = os.path.join(out_dir, "libtdr_hip_tl.so")
    b.OBJ_DIR = os.path.join(out_dir, "_obj_tl")
    b.STAMP = os.path.join(out_dir, "libtdr_hip_tl.toolchain.txt")
    print(b.build(force=True, extra_flags=["-DTDR_SCORE_TIMELINE"]))


def read_timeline(lib, name):
    fn = getattr(lib, name)
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], C.c_int
    buf = np.zeros(2 * TL_MAX, np.uint64)
    assert fn(buf.ctypes.data_as(C.c_void_p), TL_MAX) == 0, name
    t = buf.reshape(-1, 2).astype(np.int64)
    return t[(t[:, 0] > 0) & (t[:, 1] > 0)] / 100.0   # microseconds (100 MHz)


def report(name, t, capacity=None):
    if len(t) == 0:
        print(f"{name}: no workgroup left a stamp")
        return
    t0 = t[:, 0].min()
    s, e = t[:, 0] - t0, t[:, 1] - t0
    end, last = e.max(), s.max()
    life = e - s
    # resident workgroups as a step function of time
    ev = np.concatenate([np.stack([s, np.ones_like(s)], 1), np.stack([e, -np.ones_like(e)], 1)])
    ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]
    tt, res = ev[:, 0], np.cumsum(ev[:, 1])
    peak = int(res.max())
    cap = capacity or peak
    print(f"== {name}: {len(t)} live workgroups, kernel span {end:.1f} us")
    print(f"   workgroup lifetime us: mean {life.mean():.1f}  std {life.std():.1f}  min {life.min():.1f}  median "
          f"{np.median(life):.1f}  p95 {np.percentile(life, 95):.1f}  max {life.max():.1f}")
    print(f"   resident workgroups: peak {peak}, capacity taken as {cap}"
          + (f" ({len(t) / cap:.2f} rounds)" if cap else ""))
    edges = np.linspace(0.0, end, 41)
    line = []
    for a, b in zip(edges[:-1], edges[1:]):
        mid = 0.5 * (a + b)
        line.append(int(((s <= mid) & (e > mid)).sum()))
    print("   resident at the middle of 40 equal time slices:")
    for i in range(0, 40, 10):
        print("     t=%7.1f us: " % (0.5 * (edges[i] + edges[i + 1])) + " ".join("%5d" % v for v in line[i:i + 10]))
    # the run-down: from the last dispatch to the kernel's end
    sel = tt >= last
    ts = np.concatenate([[last], tt[sel], [end]])
    rs = np.concatenate([[res[~sel][-1] if (~sel).any() else 0], res[sel], [0]])
    dt = np.diff(ts)
    r = np.minimum(rs[:-1], cap)
    idle_area = float(((cap - r) * dt).sum())
    frac = 6.0 * r / cap
    rate = np.interp(frac, np.arange(7), RATE)
    lost_us = float(((1.0 - rate) * dt).sum())
    print(f"   last workgroup dispatched at {last:.1f} us; the run-down lasts {end - last:.1f} us "
          f"({100 * (end - last) / end:.1f} % of the kernel)")
    print(f"   IDLE AREA of the run-down: {idle_area:.0f} workgroup-slots x us = {idle_area / cap:.1f} us of the whole chip "
          f"empty; {lost_us / 1000:.4f} ms at full rate (the occupancy table)")
    # the same for the ramp-up, for scale: until the first workgroup ends nothing is idle but the dispatcher's own pace
    first_end = e.min()
    print(f"   first workgroup ends at {first_end:.1f} us; resident then {int(((s <= first_end) & (e > first_end)).sum())}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", default="", metavar="DIR", help="build the diagnostic library into DIR and exit")
    ap.add_argument("--config", default="c2")
    ap.add_argument("--tail", default="", help="K,Q for tdr_config_tuning su_tail_groups / su_tail_parts (default: the library's)")
    ap.add_argument("--tuning", default="", help="name=value[,name=value...] for tdr_config_tuning")
    a = ap.parse_args()
    if a.build:
        return build(a.build)
    import torch
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import synth
    from top_down_renderer_amd.kernels import HipKernels

    k = HipKernels()
    if not hasattr(k.lib, "tdr_debug_read_timeline_su"):
        raise SystemExit("not a -DTDR_SCORE_TIMELINE build: see the top of this file")
    tune = [kv.partition("=")[::2] for kv in filter(None, a.tuning.split(","))]
    if a.tail:
        kk, _, qq = a.tail.partition(",")
        tune += [("su_tail_groups", kk), ("su_tail_parts", qq)]
    for name, val in tune:
        if k.lib.tdr_config_tuning(name.encode(), int(val)) < 0:
            raise SystemExit(f"unknown knob {name!r}")
    cfg = synth.CONFIGS[a.config]
    n = cfg.n_particles // 8 if cfg.name in ("c3", "c5") else cfg.n_particles
    sc = synth.make_scene(cfg, n_particles=n)
    m = pkg.TopDownMapPolar(pkg.Params(resolution=cfg.map_resolution), sc.class_maps, sc.class_mask, kernels=k)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    r = pkg.ScanRendererPolar(sc.lut, kernels=k)
    r.set_output_shape(cfg.ncls, cfg.nb, cfg.nr)
    r.renderSemanticTopDown(torch.from_numpy(sc.pts).to(k.device), cfg.res, cfg.ang_res)
    f = pkg.ParticleFilter(n, m, pkg.FilterParams(fixed_scale=1.0), seed=1, kernels=k, locality_every=1, init_particles=False)
    f.set_states(sc.states)
    perm = k.zeros((f.cap_local,), torch.int32)
    k.locality_order(f.st, n, m.rows, m.cols, perm)

    def score():
        # (a fresh context like the one bench.py's `shares` call uses: the table's factors, the configured span)
        k.score(m.dev, r.last_scan()[1], float(cfg.res), f.fp_c, f.st, n, f.raw_w, perm=perm, uniform_scale=f._uniform_scale,
                n_total=n, ctx=k.score_ctx_create())
        k.synchronize()

    for _ in range(3):
        score()
    for name in ("tdr_debug_read_timeline_su", "tdr_debug_read_timeline_ray"):
        read_timeline(k.lib, name)        # (reading clears)
    score()
    K, Q = (int(k.lib.tdr_config_tuning(x, -1)) for x in (b"su_tail_groups", b"su_tail_parts"))
    print(f"config {cfg.name}: {n} particles, {cfg.nb} x {cfg.nr} bins; su_tail_groups {K}, su_tail_parts {Q}; "
          f"su_group {int(k.lib.tdr_config_tuning(b'su_group', -1))} (0: from the shapes)")
    # score_polar_su_kernel: 80 VGPRs and 20 KB of LDS, six workgroups of four waves per compute unit
    report("score_polar_su_kernel (dense particles)", read_timeline(k.lib, "tdr_debug_read_timeline_su"), capacity=6 * 256)
    report("score_polar_ray_kernel (scattered particles)", read_timeline(k.lib, "tdr_debug_read_timeline_ray"))


if __name__ == "__main__":
    main()
