"""NumPy restatement of the pose-grid search (include/tdr.h, "pose-grid search"): the list of lattice points, the
candidates, the reduction over headings and the peaks.  Written from the definition, not from the kernels; the GPU tests
hold the library to it with ==.  The weights come from a `score` callable, as in tests/sensor_reset_ref.py.  Not a test
module."""
from collections import namedtuple

import numpy as np

from recovery_ref import STATE_DTYPE

F32 = np.float32
NAN = np.uint32(0x7FC00000).view(F32)          # the NaN of unlisted points
PEAK_DTYPE = np.dtype([("g", "<i4"), ("cell", "<u4"), ("w", "<f4"), ("theta", "<f4")])
# the fields of tdr_grid_spec, in its order
Spec = namedtuple("Spec", "c0 r0 step nx ny road_only heading_mode n_headings theta0 dtheta scale",
                  defaults=(1, 0, 1, 0.0, 0.0, 1.0))


def cells(spec):
    """(c, r) of every lattice point g = iy * nx + ix, as int64 arrays of nx * ny."""
    g = np.arange(spec.nx * spec.ny, dtype=np.int64)
    iy, ix = g // spec.nx, g % spec.nx
    return spec.c0 + ix * spec.step, spec.r0 + iy * spec.step


def lattice_list(class_maps, spec):
    """The listed g, ascending (int32): the cell is inside the (ncls, rows, cols) map and, with road_only, a road cell (its
    class-1 value is below 1)."""
    maps = np.asarray(class_maps, F32)
    rows, cols = maps.shape[1:]
    c, r = cells(spec)
    ok = (c >= 0) & (r >= 0) & (c < cols) & (r < rows)
    if spec.road_only:
        ok[ok] = maps[1][r[ok], c[ok]] < F32(1)
    return np.flatnonzero(ok).astype(np.int32)


def candidates(spec, lst, resolution):
    """The (len(lst), H) candidate states of the listed points lst."""
    c, r = cells(spec)
    H = spec.n_headings
    out = np.zeros((len(lst), H), STATE_DTYPE)
    out["init_x_px"] = ((c[lst].astype(F32) + F32(0.5)) * F32(resolution))[:, None]      # float32 at every step
    out["init_y_px"] = ((r[lst].astype(F32) + F32(0.5)) * F32(resolution))[:, None]
    out["scale"] = F32(spec.scale)
    if spec.heading_mode == 1:
        out["theta"] = (F32(spec.theta0) + np.arange(H).astype(F32) * F32(spec.dtheta))[None, :]
        out["have_init"] = 1
    return out


def pick(w):
    """The smallest h of the largest key per row; a NaN's key is -1."""
    key = np.where(np.isnan(w), F32(-1), w)
    return np.argmax(key, axis=1)          # the first maximum


def reduce(spec, lst, w, after):
    """W, T (nx * ny) and vol (H, nx * ny) from the weights w (len(lst), H) and the states as scoring left them."""
    G, H = spec.nx * spec.ny, spec.n_headings
    W, T, vol = np.full(G, NAN, F32), np.full(G, NAN, F32), np.full((H, G), NAN, F32)
    if len(lst):
        w = np.asarray(w, F32).reshape(len(lst), H)
        h = pick(w)
        rows = np.arange(len(lst))
        W[lst] = w[rows, h]
        won = after.reshape(len(lst), H)[rows, h]
        T[lst] = np.where(won["have_init"] != 0, won["theta"], NAN)
        vol[:, lst] = w.T
    return W, T, vol


def peaks(spec, cols, W, T, R, K):
    """(the first min(K, n_peaks) peaks in the order (w descending, g ascending), n_peaks).  Written as the definition reads:
    every eligible point against every other point of its window."""
    nx, ny = spec.nx, spec.ny
    Wp = np.asarray(W, F32).reshape(ny, nx)
    elig = Wp > 0                                           # NaN, 0 and negative values are not eligible
    gg = np.arange(nx * ny, dtype=np.int64).reshape(ny, nx)
    found = []
    with np.errstate(invalid="ignore"):
        for iy, ix in zip(*np.nonzero(elig)):
            win = (slice(max(0, iy - R), min(ny, iy + R + 1)), slice(max(0, ix - R), min(nx, ix + R + 1)))
            g, v = gg[iy, ix], Wp[iy, ix]
            others = elig[win] & (gg[win] != g)
            passes = (Wp[win] < v) | ((Wp[win] == v) & (gg[win] > g))
            if not (others & ~passes).any():
                found.append(g)
    found = np.array(found, np.int64)
    order = np.lexsort((found, -Wp.ravel()[found].astype(np.float64))) if len(found) else np.zeros(0, np.int64)
    top = found[order][:K]
    c, r = cells(spec)
    out = np.zeros(len(top), PEAK_DTYPE)
    out["g"] = top
    out["cell"] = r[top] * cols + c[top]
    out["w"] = Wp.ravel()[top]
    out["theta"] = np.asarray(T, F32).ravel()[top]
    return out, len(found)


def grid_search(class_maps, resolution, spec, score, R, K):
    """The whole definition.  score(candidates (m,) STATE_DTYPE) -> (weights (m,), the states as scoring left them).
    Returns (W, T, vol, peaks, n_peaks, the list)."""
    lst = lattice_list(class_maps, spec)
    cand = candidates(spec, lst, resolution)
    if len(lst):
        w, after = score(np.ascontiguousarray(cand.reshape(-1)))
    else:
        w, after = np.zeros(0, F32), cand.reshape(-1)
    W, T, vol = reduce(spec, lst, w, after)
    pk, n_peaks = peaks(spec, np.asarray(class_maps).shape[2], W, T, R, K)
    return W, T, vol, pk, n_peaks, lst
