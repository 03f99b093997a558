#!/usr/bin/env python3
"""Times map fusion (include/tdr.h, "map fusion"; csrc/tdr_fuse.hip, csrc/tdr_host_fuse.cpp) at the shape of config 2: a
4000 x 4000 six-class label map, 256 x 256 polar renders of a 100 000-point scan.
  - the vote launch for 1, 16 and 64 scans (device events around the launcher) and the handle's add / add_batch (wall
    clock: job upload, launch, read-back of the two counters);
  - the label pass over the tiles those scans dirtied (events);
  - apply end to end (wall) with a changed block of 256^2 and 1024^2 cells, against the only route to the same end state
    without the fuser: tdr_map_update_labels_incremental with a full image composed on the host (composition included).
Medians of `reps`; every shape is warmed up once.  Writes the lines it prints to `out` as well.
    python3 tools/time_fuse.py [out = profiles/time_fuse_v1.txt] [size = 4000] [reps = 7]"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from top_down_renderer_amd import batch, synth  # noqa: E402
from top_down_renderer_amd._lib import FuseJobC, check  # noqa: E402
from top_down_renderer_amd.fuse import MapFuser  # noqa: E402
from top_down_renderer_amd.kernels import DeviceMap, HipKernels  # noqa: E402


def wall(fn, reps, before=None):
    ts = []
    for _ in range(reps + 1):                      # the first one warms up
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[1:])), float(min(ts[1:])), float(max(ts[1:]))


def events(fn, reps, inner=20):
    """ms per call: `inner` calls between two events (one launch is far below the event resolution's comfort)"""
    ts = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return float(np.median(ts[1:])), float(min(ts[1:])), float(max(ts[1:]))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "time_fuse_v1.txt")
    size = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cfg = synth.CONFIGS["c2"]
    ncls, nb, nr, res = cfg.ncls, cfg.nb, cfg.nr, 1.0
    rng = np.random.default_rng(cfg.seed)
    lab = synth.make_label_image(size, ncls, rng)
    img = np.where(lab < 0, 255, lab).astype(np.uint8)[::-1].copy()
    lut = synth.make_lut(ncls)
    cl = np.arange(ncls, dtype=np.uint8)
    k = HipKernels()
    L, vp = k.lib, C.c_void_p
    say(f"map {size} x {size}, {ncls} classes, resolution {res}; polar render {nb} x {nr} of {cfg.n_pts} points; "
        f"median [min, max] of {reps}; {torch.cuda.get_device_name(0)}")

    m = batch.MapHandle.from_labels(img, lut, ncls, res)
    m.sample_pts_polar(nb, nr, cfg.ang_res)
    margin = min(size // 4, 300)
    poses = [synth.pick_true_pose(lab, rng, margin) for _ in range(64)]
    renderers = []
    for pose in poses:
        r = batch.Renderer(lut)
        pts = synth.make_scan(cfg, lab, pose, rng)
        r.render_polar(pts, 4, 3, cfg.res, cfg.ang_res, ncls, nb, nr)
        renderers.append(r)
    render0, _ = renderers[0].get_render()
    nonzero = int((render0 > 0).any(0).sum())
    say(f"one render: {nonzero} of {nb * nr} bins hold a count in some class, {int(render0.sum())} votes")
    p5 = [(p[0], p[1], p[2], 1.0, cfg.res) for p in poses]

    # ---- the vote launch alone: the launchers over torch tensors ----
    dm = DeviceMap(k.zeros((4,)), ncls, size, size, res)
    k.set_polar_table(dm, nb, nr, cfg.ang_res)
    votes, dirty, counters = k.fuse_state(dm)
    scans = [k.to_device(np.ascontiguousarray(r.get_render()[0].transpose(0, 2, 1))) for r in renderers]
    jobs = {}
    for kk in (16, 64):                             # the device job array of a batch, built once like a caller would keep it
        arr = (FuseJobC * kk)()
        for j, s, p in zip(arr, scans, p5):
            j.scan, j.rows, j.cols, j.polar = s.data_ptr(), nb, nr, 1
            j.cx, j.cy, j.theta, j.scale, j.res = p
        jobs[kk] = k.to_device(np.frombuffer(bytearray(arr), np.uint8))

    def launch_one():
        k.fuse_votes(dm, scans[:1], [True], p5[:1], votes, dirty, counters)

    def launch_jobs(kk):
        check(L.tdr_k_fuse_votes_jobs(C.byref(dm.desc), vp(dm.tab.data_ptr()), nb, nr, vp(jobs[kk].data_ptr()), kk, nb * nr,
                                      vp(votes.data_ptr()), vp(dirty.data_ptr()), vp(counters.data_ptr()), k.stream()))
    t = events(launch_one, reps)
    say(f"vote launch, 1 scan (tdr_k_fuse_votes): {t[0] * 1e3:.1f} us [{t[1] * 1e3:.1f}, {t[2] * 1e3:.1f}] (events, 20 launches each)")
    for kk in (16, 64):
        t = events(lambda: launch_jobs(kk), reps)
        say(f"vote launch, {kk} scans (tdr_k_fuse_votes_jobs): {t[0] * 1e3:.1f} us [{t[1] * 1e3:.1f}, {t[2] * 1e3:.1f}] (events)")
    # the label pass over what 16 scans dirtied
    votes.zero_()
    dirty.zero_()
    launch_jobs(16)
    bits = dirty.cpu().numpy().view(np.uint32)
    tiles = k.to_device(np.asarray([t for t in range(32 * len(bits)) if bits[t >> 5] >> (t & 31) & 1], np.int32))
    base = k.to_device(img)
    current = base.clone()
    t = events(lambda: k.fuse_labels(votes, img.shape, res, cl, 3, (1, 2), base, current, tiles), reps, inner=1)
    say(f"label pass over the {tiles.numel()} tiles 16 scans dirtied (tdr_k_fuse_labels + the 20-byte result read back): "
        f"{t[0] * 1e3:.1f} us [{t[1] * 1e3:.1f}, {t[2] * 1e3:.1f}] (events)")
    del votes, dirty, base, current, scans

    # ---- the handle ----
    fuser = MapFuser(m, cl, 3, (1, 2))
    t = wall(lambda: fuser.add_scan(renderers[0], p5[0][:4], cfg.res), reps)
    say(f"tdr_fuser_add, 1 robot: {t[0]:.3f} ms [{t[1]:.3f}, {t[2]:.3f}] (wall: job upload, launch, counters read back)")
    for kk in (16, 64):
        t = wall(lambda: fuser.add_scans(renderers[:kk], p5[:kk]), reps)
        say(f"tdr_fuser_add_batch, {kk} robots: {t[0]:.3f} ms [{t[1]:.3f}, {t[2]:.3f}] (wall)")
    fuser.reset()
    fuser.apply()

    # ---- apply end to end against the host-composed full image ----
    ch = C.c_int64(0)
    for side in (256, 1024):
        y0 = x0 = size // 3                                           # map cell of the block's corner
        block = np.zeros((ncls, side, side), np.float32)
        block[0] = 5                                                  # every cell of the block gets a verdict for class 0
        centre = (x0 + (side - 1) / 2.0, y0 + (side - 1) / 2.0, 0.0, 1.0)

        def prepare():
            fuser.reset()
            fuser.apply()                                             # back to the base image
            fuser.add_images(block, False, centre, 1.0)
        t = wall(lambda: ch.__setattr__("value", fuser.apply()), reps, before=prepare)
        changed = ch.value
        fused = fuser.labels()
        ys, xs = np.nonzero(fused != img)
        say(f"apply, votes on a block of {side} x {side} cells ({changed} cells changed, rectangle "
            f"{ys.max() - ys.min() + 1} x {xs.max() - xs.min() + 1}): {t[0]:.2f} ms [{t[1]:.2f}, {t[2]:.2f}] (wall: "
            f"dirty bitmap read back, label pass, rectangle read back, tdr_map_patch_labels)")
        fuser.reset()
        fuser.apply()
        patch = fused[ys.min():ys.max() + 1, xs.min():xs.max() + 1].copy()
        state = {}

        def restore():
            check(L.tdr_map_update_labels_incremental(m.h, img.ctypes.data_as(vp), size, size, lut.ctypes.data_as(vp), 256,
                                                      ncls, C.c_float(res), 0, 0, C.byref(ch)))

        def host_route():
            new = img.copy()                                          # the caller's full image with the block composed in
            new[ys.min():ys.max() + 1, xs.min():xs.max() + 1] = patch
            state["new"] = new
            check(L.tdr_map_update_labels_incremental(m.h, new.ctypes.data_as(vp), size, size, lut.ctypes.data_as(vp), 256,
                                                      ncls, C.c_float(res), 0, 0, C.byref(ch)))
        t = wall(host_route, reps, before=restore)
        say(f"  the same end state without the fuser: host-composed full image + tdr_map_update_labels_incremental "
            f"({ch.value} cells changed): {t[0]:.2f} ms [{t[1]:.2f}, {t[2]:.2f}] (wall, composition included)")
        restore()
        assert fuser.rebase()

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
