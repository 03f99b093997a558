"""NumPy restatement of the recovery injection (include/tdr.h, "recovery injection"): Philox4x32-10, the road list of a map,
the injection of a particle set and the slow / fast average tracker.  Written from the definition, not from the kernels;
the GPU tests hold the library to it with ==.  Not a test module."""
import math

import numpy as np

F32 = np.float32
U64 = np.uint64
M32 = U64(0xFFFFFFFF)
STATE_DTYPE = np.dtype([("init_x_px", "<f4"), ("init_y_px", "<f4"), ("dx_m", "<f4"), ("dy_m", "<f4"), ("theta", "<f4"),
                        ("scale", "<f4"), ("have_init", "u1"), ("pad", "u1", 3)])


def philox(counter, key):
    """Philox4x32-10.  counter: 4 words, key: 2 words, each a scalar or an array (broadcast together).  Returns a uint32 array
    of shape (4,) + the broadcast shape."""
    c = [np.asarray(v, U64) & M32 for v in counter]
    k = [np.asarray(v, U64) & M32 for v in key]
    shape = np.broadcast(*c, *k).shape
    c = [np.broadcast_to(v, shape).copy() for v in c]
    k = [np.broadcast_to(v, shape).copy() for v in k]
    for _ in range(10):
        p0 = U64(0xD2511F53) * c[0]          # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = U64(0xCD9E8D57) * c[2]
        c = [(p1 >> U64(32)) ^ c[1] ^ k[0], p1 & M32, (p0 >> U64(32)) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + U64(0x9E3779B9)) & M32, (k[1] + U64(0xBB67AE85)) & M32]
    return np.stack(c).astype(np.uint32)


def threshold(p):
    """threshold24 of a probability: floor(p * 2^24) in double, clamped to [0, 2^24]; a NaN gives 0."""
    v = math.floor(p * 16777216.0) if math.isfinite(p) else (16777216 if p > 0 else 0)
    return int(min(max(v, 0), 16777216))


def road_cells(class_maps):
    """class_maps: (ncls, rows, cols) distance maps indexed [cls, row, col].  The ascending cell indices r * cols + c of the
    cells whose class-1 value is below 1 (the on-road test of particle initialisation)."""
    return np.flatnonzero(np.asarray(class_maps, F32)[1].ravel() < F32(1)).astype(np.uint32)


def inject(states, n, slot_begin, road, cols, resolution, seed, draw, threshold24, heading_mode):
    """The injection of slots [0, n) of `states` (a STATE_DTYPE array, not changed).  Returns (the new array, the number of
    injected slots).  Slots behind n and slots that are not injected come back as they were."""
    out = states.copy()
    if n == 0 or threshold24 == 0:
        return out, 0
    road = np.asarray(road, np.uint32)
    i = (np.arange(n, dtype=U64) + U64(slot_begin)) & M32
    key = (seed & 0xFFFFFFFF, seed >> 32)
    d = (draw & 0xFFFFFFFF, draw >> 32)
    a = philox((i, d[0], d[1], 0), key)
    sel = (a[0] >> np.uint32(8)) < np.uint32(threshold24) if threshold24 < (1 << 24) else np.ones(n, bool)
    cell = road[((a[1].astype(U64) * U64(len(road))) >> U64(32)).astype(np.int64)]
    r, c = cell // np.uint32(cols), cell % np.uint32(cols)
    ux = (a[2] >> np.uint32(24)).astype(F32) * F32(2.0 ** -8)
    uy = (a[3] >> np.uint32(24)).astype(F32) * F32(2.0 ** -8)
    x = (c.astype(F32) + ux) * F32(resolution)       # float32 at every step
    y = (r.astype(F32) + uy) * F32(resolution)
    if heading_mode == 1:
        b = philox((i, d[0], d[1], 1), key)
        theta = (b[0] >> np.uint32(8)).astype(F32) * F32(2.0 ** -24) * F32(6.2831855) - F32(3.1415927)
        have = 1
    else:
        theta, have = np.zeros(n, F32), 0
    idx = np.flatnonzero(sel)
    out["init_x_px"][idx] = x[idx]
    out["init_y_px"][idx] = y[idx]
    out["dx_m"][idx] = 0
    out["dy_m"][idx] = 0
    out["theta"][idx] = theta[idx]
    out["have_init"][idx] = have
    return out, len(idx)


def on_road(class_maps, resolution, x, y):
    """The StateParticle constructor's on-road test (getClassesAtPoint for class 1) of positions x, y in map pixels."""
    m1 = np.asarray(class_maps, F32)[1]
    ix, iy = np.asarray(x, F32).astype(np.int32), np.asarray(y, F32).astype(np.int32)
    c0 = (ix.astype(F32) / F32(resolution)).astype(np.int32)
    c1 = (iy.astype(F32) / F32(resolution)).astype(np.int32)
    inside = (c0 >= 0) & (c1 >= 0) & (c0 < m1.shape[1]) & (c1 < m1.shape[0])
    ok = np.zeros(len(ix), bool)
    ok[inside] = m1[c1[inside], c0[inside]] < F32(1)
    return ok


class Tracker:
    """The slow and the fast average of the updates' mean raw weight (double)."""

    def __init__(self, alpha_slow, alpha_fast, p_max):
        self.alpha_slow, self.alpha_fast, self.p_max = float(alpha_slow), float(alpha_fast), float(p_max)
        self.w_slow = self.w_fast = 0.0

    def track(self, w_avg):
        w_avg = float(w_avg)
        if not math.isfinite(w_avg) or not w_avg > 0.0:
            return 0.0
        self.w_slow = w_avg if self.w_slow == 0.0 else self.w_slow + self.alpha_slow * (w_avg - self.w_slow)
        self.w_fast = w_avg if self.w_fast == 0.0 else self.w_fast + self.alpha_fast * (w_avg - self.w_fast)
        return min(self.p_max, max(0.0, 1.0 - self.w_fast / self.w_slow))

    def reset(self):
        self.w_slow = self.w_fast = 0.0
