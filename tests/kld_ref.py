"""NumPy restatement of the KLD-sampling count (include/tdr.h, "KLD-sampling count"): the checker of tests/test_kld.py,
itself checked against hand-worked facts by tests/test_kld_ref.py.  Not a test module.

Every float expression is float32, rounding for rounding; the heading bin is np_oracle.rot_shift, the scale bin an integer
shift of the scale's bits, k is np.unique."""
import math
from dataclasses import dataclass

import numpy as np

from oracle import np_oracle as no

F32 = np.float32
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
BIN_LO, BIN_HI = F32(-524288.0), F32(524287.0)


@dataclass
class Params:
    bin_xy_px: float = 4.0
    theta_bins: int = 36
    scale_bits: int = 3
    epsilon: float = 0.05
    z: float = 2.326
    n_min: int = 100

    def to_c(self):
        from top_down_renderer_amd._lib import KldParamsC
        return KldParamsC(self.bin_xy_px, self.theta_bins, self.scale_bits, self.epsilon, self.z, self.n_min)


def centre(states):
    """(cx, cy, s) of a structured array of States: the scorer's centre, two float32 roundings each."""
    s = states["scale"].astype(F32)
    with np.errstate(all="ignore"):
        cx = (states["dx_m"].astype(F32) * s).astype(F32) + states["init_x_px"].astype(F32)
        cy = (states["dy_m"].astype(F32) * s).astype(F32) + states["init_y_px"].astype(F32)
    return cx.astype(F32), cy.astype(F32), s


def pos_bin(c, bin_xy_px):
    """floor(med3(c / bin, -2^19, 2^19 - 1)) of finite float32 c, as int64."""
    with np.errstate(all="ignore"):
        q = (np.asarray(c, F32) / F32(bin_xy_px)).astype(F32)
    return np.floor(np.clip(q, BIN_LO, BIN_HI)).astype(np.int64)


def scale_bin(s, scale_bits):
    return (np.asarray(s, F32).view(np.uint32) >> np.uint32(23 - scale_bits)).astype(np.int64)


def keys(states, params):
    """uint64 (n,): the key of every particle, NO_KEY where it has none."""
    n = len(states)
    out = np.full(n, NO_KEY, np.uint64)
    if n == 0:
        return out
    cx, cy, s = centre(states)
    with np.errstate(all="ignore"):
        ok = np.isfinite(cx) & np.isfinite(cy) & np.isfinite(s) & (s > 0)
    ix = pos_bin(np.where(ok, cx, F32(0)), params.bin_xy_px)
    iy = pos_bin(np.where(ok, cy, F32(0)), params.bin_xy_px)
    T = int(params.theta_bins)
    it = np.full(n, T, np.int64)
    th = states["theta"].astype(F32)
    sel = np.nonzero(ok & (states["have_init"] != 0))[0]
    uth, inv = np.unique(th[sel].view(np.uint32), return_inverse=True)   # (one call per distinct heading)
    it[sel] = np.asarray([no.rot_shift(t, T) for t in uth.view(F32)], np.int64)[inv] if len(sel) else 0
    isc = scale_bin(np.where(ok, s, F32(1)), params.scale_bits)
    key = ((ix + 524288).astype(np.uint64) << np.uint64(43)) | ((iy + 524288).astype(np.uint64) << np.uint64(23)) | \
        (it.astype(np.uint64) << np.uint64(14)) | isc.astype(np.uint64)
    out[ok] = key[ok]
    return out


def count(states, n, params):
    """(k, skipped) of particles [0, n)."""
    kk = keys(states[:n], params)
    have = kk != NO_KEY
    return int(len(np.unique(kk[have]))), int((~have).sum())


def bound(k, eps, z):
    """Fox's bound in double, in the header's order; 0 for k < 2; saturated at 2^62."""
    if k < 2:
        return 0
    a = 2.0 / (9.0 * (k - 1))
    t = 1.0 - a + math.sqrt(a) * z
    v = math.ceil(((k - 1) / (2.0 * eps)) * (t * t * t))
    return min(int(v), 1 << 62)


def target(n_kld, last_count, n_min, max_count):
    return min(max(n_kld, n_min, 3 * last_count // 4 + 10), max_count)


def target_of(states, n, params, max_count):
    """The next update's count of a filter holding states[:n]: (k, skipped, target)."""
    k, sk = count(states, n, params)
    return k, sk, target(bound(k, params.epsilon, params.z), n, params.n_min, max_count)
