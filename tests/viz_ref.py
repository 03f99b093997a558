"""What the particle picture (include/tdr.h, "the particle picture") must be, restated in NumPy and
Python's math, which calls the same host libm as the library's host code (shared by tests/test_viz_ref.py and
tests/test_viz.py; not a test module).

  * a segment's pixels: the integer coverage rule, evaluated over the segment's clipped bounding box;
  * Arrow, Disc, the ellipse polyline: double arithmetic in the definition's order, round() = lrint (half to even);
  * float -> int: x86's rule (INT_MIN for NaN and outside int's range);
  * cosf / sinf: the library's host restatement of the host libm (tests/test_libm.py pins it), the variant this host takes;
  * per-particle float32 expressions with two roundings (no contraction);
  * particles are deduplicated by (kind, pt, dir) before stamping, so a converged cloud of 100 000 costs nothing.

Nothing here imports the package's kernels."""
import ctypes as C
import math

import numpy as np

F32 = np.float32
INT_MIN = -2 ** 31
LIM = 1 << 20            # overlay endpoints beyond +-2^20 are not drawn
RED, GREEN, BLUE = (0, 0, 255), (0, 255, 0), (255, 0, 0)
PLANE_COLOURS = (RED, GREEN, BLUE, GREEN)   # arrows, dots, mixture + best, caller's arrows: later over earlier
FIELDS = ("init_x_px", "init_y_px", "dx_m", "dy_m", "theta", "scale")


def f2i(v):
    """(int)v of a float32 on x86-64."""
    v = F32(v)
    return int(v) if -2147483648.0 <= v < 2147483648.0 else INT_MIN


def f2i_array(v):
    """f2i over a float32 array, int64."""
    v = np.asarray(v, F32)
    with np.errstate(invalid="ignore"):
        ok = (v >= F32(-2147483648.0)) & (v < F32(2147483648.0))
    out = np.full(v.shape, INT_MIN, np.int64)
    out[ok] = np.trunc(v[ok]).astype(np.int64)
    return out


def sincos(theta):
    """The host libm's sinf / cosf as the library restates them (the variant this host's libm takes)."""
    from top_down_renderer_amd import _lib
    L = _lib.load()
    v = L.tdr_libm_variant()
    assert v in (0, 1)
    x = np.ascontiguousarray(theta, F32).reshape(-1)
    s, c = np.empty_like(x), np.empty_like(x)
    assert L.tdr_sincosf_host(x.ctypes.data_as(C.c_void_p), len(x), v, s.ctypes.data_as(C.c_void_p),
                              c.ctypes.data_as(C.c_void_p)) == 0
    return s, c


def dirs(theta):
    """dir = ((int)(cosf(theta) * 5), (int)(-sinf(theta) * 5)) per heading, int64 (n, 2); rows of non-finite headings
    are meaningless (callers mask them)."""
    s, c = sincos(theta)
    with np.errstate(invalid="ignore"):
        dx = np.trunc(np.nan_to_num(c * F32(5))).astype(np.int64)
        dy = np.trunc(np.nan_to_num(-s * F32(5))).astype(np.int64)
    return np.stack([dx, dy], axis=1)


# ---- primitives -----------------------------------------------------------------------------------------------------
def covered(ax, ay, bx, by, px, py):
    """The coverage rule for one pixel, in Python integers (exact at any size)."""
    ux, uy, wx, wy = bx - ax, by - ay, px - ax, py - ay
    L, d = ux * ux + uy * uy, ux * wx + uy * wy
    if L == 0 or d <= 0:
        return wx * wx + wy * wy <= 1
    if d >= L:
        return (px - bx) ** 2 + (py - by) ** 2 <= 1
    return (ux * wy - uy * wx) ** 2 <= L


def segment_pixels(ax, ay, bx, by, x_lo, x_hi, y_lo, y_hi):
    """(xs, ys) of the pixels of segment A -> B inside [x_lo, x_hi] x [y_lo, y_hi] (inclusive), vectorised; the
    endpoints are within +-2^20, so int64 holds every product once |cross| is bounded."""
    x0, x1 = max(min(ax, bx) - 1, x_lo), min(max(ax, bx) + 1, x_hi)
    y0, y1 = max(min(ay, by) - 1, y_lo), min(max(ay, by) + 1, y_hi)
    if x0 > x1 or y0 > y1:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    py, px = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64), indexing="ij")
    ux, uy, wx, wy = bx - ax, by - ay, px - ax, py - ay
    L, d = ux * ux + uy * uy, ux * wx + uy * wy
    near_a = wx * wx + wy * wy <= 1
    near_b = (px - bx) ** 2 + (py - by) ** 2 <= 1
    c = np.abs(ux * wy - uy * wx)
    small = c < (1 << 22)                       # c^2 <= L < 2^44 needs c < 2^22
    mid = small & (np.where(small, c, 0) ** 2 <= L)
    cov = np.where((L == 0) | (d <= 0), near_a, np.where(d >= L, near_b, mid))
    return px[cov], py[cov]


def arrow(x1, y1, x2, y2):
    """The three segments of Arrow(p1, p2): the shaft, the tip at ang + pi/4, the tip at ang - pi/4."""
    dx, dy = float(x1 - x2), float(y1 - y2)
    tip = math.sqrt(dx * dx + dy * dy) * 0.3
    ang = math.atan2(dy, dx)
    segs = [(x1, y1, x2, y2)]
    for a in (ang + math.pi / 4, ang - math.pi / 4):
        segs.append((round(float(x2) + tip * math.cos(a)), round(float(y2) + tip * math.sin(a)), x2, y2))
    return segs


_STAMPS = {}


def arrow_stamp(dx, dy):
    """Offsets (k, 2) of the pixels of Arrow(-dir, dir) about the origin."""
    key = (int(dx), int(dy))
    if key not in _STAMPS:
        pts = set()
        for s in arrow(-key[0], -key[1], key[0], key[1]):
            xs, ys = segment_pixels(*s, -16, 16, -16, 16)
            pts.update(zip(xs.tolist(), ys.tolist()))
        _STAMPS[key] = np.asarray(sorted(pts), np.int64).reshape(-1, 2)
    return _STAMPS[key]


DISC = np.asarray([(x, y) for y in range(-2, 3) for x in range(-2, 3) if x * x + y * y <= 5], np.int64)


# ---- layers -----------------------------------------------------------------------------------------------------------
def _fields(st):
    if getattr(st, "dtype", None) is not None and st.dtype.names:
        return [np.ascontiguousarray(st[f], F32) for f in FIELDS]
    return [np.ascontiguousarray(st[i], F32) for i in range(6)]


def particle_points(st, H, W):
    """Per particle: pt (n, 2) as Python-exact int64, inside (n,), dir (n, 2), finite heading (n,)."""
    ix, iy, dx, dy, th, sc = _fields(st)
    with np.errstate(all="ignore"):
        x = (dx * sc).astype(F32) + ix
        y = F32(H) - ((dy * sc).astype(F32) + iy).astype(F32)
    px, py = f2i_array(x), f2i_array(y)
    inside = ~((px < 0) | (px > W) | (py < 0) | (py > H))
    finite = np.isfinite(th)
    return np.stack([px, py], axis=1), inside, dirs(np.where(finite, th, F32(0))), finite


def _stamp(plane, offs, cx, cy):
    H, W = plane.shape
    x, y = offs[:, 0] + cx, offs[:, 1] + cy
    ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    plane[y[ok], x[ok]] = True


def particle_planes(st, H, W):
    """Planes 0 (arrows) and 1 (dots) as bool (H, W) arrays."""
    arrows, dots = np.zeros((H, W), bool), np.zeros((H, W), bool)
    if len(_fields(st)[0]) == 0:
        return arrows, dots
    pt, inside, d, finite = particle_points(st, H, W)
    sel = inside & finite
    for cx, cy, dx, dy in np.unique(np.concatenate([pt[sel], d[sel]], axis=1), axis=0):
        _stamp(arrows, arrow_stamp(dx, dy), cx, cy)
    out = pt[~inside]
    out = np.stack([np.clip(out[:, 0], 5, W - 5), np.clip(out[:, 1], 5, H - 5)], axis=1)
    for cx, cy in np.unique(out, axis=0):
        _stamp(dots, DISC, cx, cy)
    return arrows, dots


def _heading(x, y, theta, H):
    """The `arrow` of particle_viz.h at mlState (x, y, theta): segments, or none for a non-finite heading."""
    theta = F32(theta)
    if not np.isfinite(theta):
        return []
    cx, cy = f2i(x), f2i(F32(H) - F32(y))
    (dx, dy), = dirs([theta]).tolist()
    return _arrow_if_in_range(cx - dx, cy - dy, cx + dx, cy + dy)


def _in_range(*v):
    return all(-LIM <= q <= LIM for q in v)


def _arrow_if_in_range(x1, y1, x2, y2):
    return arrow(x1, y1, x2, y2) if _in_range(x1, y1, x2, y2) else []


def overlay(means, covs, best, arrows, H):
    """Layers 4 and 5 as a list of (x1, y1, x2, y2, plane), in the library's order."""
    means = np.asarray(means, F32).reshape(-1, 3)
    covs = np.asarray(covs, F32).reshape(-1, 3, 3)
    segs = []

    def push(s, plane):
        if _in_range(*s):
            segs.append(tuple(int(q) for q in s) + (plane,))

    with np.errstate(all="ignore"):
        for mean, cov in zip(means, covs):
            a, b, d = F32(cov[0, 0]), F32(cov[0, 1]), F32(cov[1, 1])
            tr = a + d
            e = (a - d) * (a - d) / F32(4) + b * b
            disc = np.sqrt(e if F32(0) < e else F32(0))
            l0, l1 = tr / F32(2) - disc, tr / F32(2) + disc
            if l0 < 0 or l1 < 0:
                break
            vx, vy = b, l0 - a
            if np.abs(vx) + np.abs(vy) < F32(1e-12):
                vx, vy = F32(1), F32(0)
            phi = float(np.arctan2(F32(-vy), F32(vx)))
            cx, cy = f2i(mean[0]), f2i(F32(H) - mean[1])
            ea, eb = float(2 * f2i(np.sqrt(l0))), float(2 * f2i(np.sqrt(l1)))
            cp, sp = math.cos(phi), math.sin(phi)
            verts = []
            for j in range(72):
                t = j * (math.pi / 36)
                ct, st = math.cos(t), math.sin(t)
                X = (float(cx) + (ea * ct) * cp) - (eb * st) * sp
                Y = (float(cy) + (ea * ct) * sp) + (eb * st) * cp
                verts.append((round(X) if abs(X) <= LIM else None, round(Y) if abs(Y) <= LIM else None))
            for j in range(72):
                s = verts[j] + verts[(j + 1) % 72]
                if None not in s:
                    push(s, 2)
            for s in _heading(mean[0], mean[1], mean[2], H):
                push(s, 2)
        if best is not None:
            for s in _heading(best[0], best[1], best[2], H):
                push(s, 2)
    for x1, y1, x2, y2 in (np.zeros((0, 4), np.int64) if arrows is None else np.asarray(arrows, np.int64).reshape(-1, 4)).tolist():
        for s in _arrow_if_in_range(x1, y1, x2, y2):
            push(s, 3)
    return segs


def segment_planes(segs, H, W):
    """Planes 2 and 3 from overlay segments."""
    planes = {2: np.zeros((H, W), bool), 3: np.zeros((H, W), bool)}
    for x1, y1, x2, y2, p in segs:
        xs, ys = segment_pixels(x1, y1, x2, y2, 0, W - 1, 0, H - 1)
        planes[p][ys, xs] = True
    return planes[2], planes[3]


def compose(background, planes):
    img = np.array(background, np.uint8, copy=True)
    for plane, colour in zip(planes, PLANE_COLOURS):
        img[plane] = colour
    return img


# ---- published size and resample ----------------------------------------------------------------------------------------
def published_size(H, W, s):
    """(out_h, out_w) = ((int)((float)H * s), (int)((float)W * s)) with a float product and x86's conversion."""
    with np.errstate(all="ignore"):
        return f2i(F32(H) * F32(s)), f2i(F32(W) * F32(s))


def _taps(n_in, n_out):
    o = np.arange(n_out, dtype=np.float64)
    f = ((o + 0.5) * (np.float64(n_in) / np.float64(n_out)) - 0.5).astype(F32)
    s = np.floor(f)
    f = (f - s).astype(F32)
    s = s.astype(np.int64)
    lo, hi = s < 0, s >= n_in - 1
    s = np.where(lo, 0, np.where(hi, n_in - 1, s))
    f = np.where(lo | hi, F32(0), f).astype(F32)
    a1 = np.rint(f * F32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, n_in - 1), 2048 - a1, a1


def resample(img, out_h, out_w):
    H, W = img.shape[:2]
    if (out_h, out_w) == (H, W):
        return img.copy()
    y0, y1, b0, b1 = _taps(H, out_h)
    x0, x1, a0, a1 = _taps(W, out_w)
    S = img.astype(np.int64)
    acc = np.zeros((out_h, out_w, 3), np.int64)
    for ys, b in ((y0, b0), (y1, b1)):
        for xs, a in ((x0, a0), (x1, a1)):
            acc += (b[:, None] * a[None, :])[:, :, None] * S[ys][:, xs]
    return ((acc + (1 << 21)) >> 22).astype(np.uint8)


def render(st, background, means=(), covs=(), best=None, arrows=None, pub_scale=1.0, layers=(0, 1, 2, 3)):
    """The published image.  layers: the planes that take part (the layer-order test removes them in turn)."""
    H, W = background.shape[:2]
    out_h, out_w = published_size(H, W, pub_scale)
    if not (1 <= out_h <= 32768 and 1 <= out_w <= 32768):
        raise ValueError("no published image")
    p0, p1 = particle_planes(st, H, W)
    p2, p3 = segment_planes(overlay(means, covs, best, arrows, H), H, W)
    planes = [p if i in layers else np.zeros((H, W), bool) for i, p in enumerate((p0, p1, p2, p3))]
    return resample(compose(background, planes), out_h, out_w)
