"""The raw weight of StateParticle::computeWeight (src/state_particle.cpp:157-219) for have_init = 1 with every sum formed
EXACTLY — the number the integer form of a scoring launch claims to give.  CPU only; not a test module.

The window comes from the oracle as it is (oracle.local_map_polar / local_map_cart), the circular shift from
oracle.rot_shift, the gates are the oracle's (orc_compute_weights; the Cartesian score has none).  What differs from the
oracle is the arithmetic of the sums alone:

* a map value is a float, i.e. an integer times a power of two.  Q is the smallest power with value * 2^Q an integer for
  every value of the map (derived here from the floats' bits); per class  sum count * value = N / 2^Q  with N an integer;
* N, the normalisation  sum count * known  and the known-cell count are formed as exact integers: 32-bit limbs of the
  products summed in uint64 and combined as Python ints — no bound on the scan's total count short of 2^32 terms;
* N / 2^Q is rounded to float32 ONCE by an integer round-half-even routine (round_to_f32), never through a double;
* from there the reference's own steps in its float / double mix, as score_finalize_exact_kernel documents them:
      cost = (float)((double)cost + (double)dot_c * 0.01 * (double)class_weight_c)      :136-139, class by class
      cost = cost / (float)normalisation                                                 :154
      w    = (float)(1. / (double)(cost + regularization))                               :212
  with NaN where fewer than half of the window's cells are known (:117-120).
"""
import numpy as np

f32 = np.float32
M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def round_to_f32(n, q=0):
    """The float32 nearest to n / 2^q (n a non-negative Python int), ties to even, in integer arithmetic."""
    n = int(n)
    assert n >= 0
    if n == 0:
        return f32(0)
    shift = n.bit_length() - 24
    if shift > 0:
        mant, rem, half = n >> shift, n & ((1 << shift) - 1), 1 << (shift - 1)
        if rem > half or (rem == half and (mant & 1)):
            mant += 1          # (2^24 is a float too)
    else:
        mant, shift = n, 0
    e = shift - int(q)
    assert -126 <= e and e + 24 <= 127, "outside the normal range of a float"
    return np.ldexp(f32(mant), e).astype(f32)   # mant <= 2^24: exact; a power of two scales exactly


def map_power(class_maps):
    """Q: the smallest q >= 0 with value * 2^q an integer for every (finite, non-negative) value of the map."""
    v = np.unique(np.asarray(class_maps, f32))
    v = v[v != 0]
    assert np.isfinite(v).all() and (v > 0).all(), "the exact reference is for finite, non-negative maps"
    if len(v) == 0:
        return 0
    bits = v.view(np.uint32).astype(np.int64)
    expo, frac = (bits >> 23) & 0xFF, bits & 0x7FFFFF
    assert (expo > 0).all(), "no subnormal map values"
    mant = frac | (1 << 23)                           # value = mant * 2^(expo - 150)
    tz = np.zeros_like(mant)
    for b in range(24):                                # trailing zeros of the 24-bit mantissa
        low = (mant >> b) & 1
        tz = np.where((tz == b) & (low == 0), b + 1, tz)
    return int(max(0, (150 - expo - tz).max()))


def exact_dot(counts, vints):
    """sum counts[k] * vints[k] as a Python int; counts < 2^32, vints < 2^64 (uint64 arrays), up to 2^32 terms."""
    counts = np.asarray(counts, np.uint64)
    vints = np.asarray(vints, np.uint64)
    assert counts.max(initial=0) <= int(M32)
    total = 0
    for limb, v in enumerate((vints & M32, vints >> S32)):
        p = counts * v                                 # < 2^64: both factors below 2^32
        part = int((p & M32).sum(dtype=np.uint64)) + (int((p >> S32).sum(dtype=np.uint64)) << 32)
        total += part << (32 * limb)
    return total


class Scan:
    """A scan image [ncls][P] of whole, non-negative counts as per-class lists of its non-empty bins."""

    def __init__(self, scan):
        scan = np.asarray(scan, f32)
        assert (scan >= 0).all() and (scan == np.floor(scan)).all() and (scan < 2.0 ** 32).all()
        self.ncls, self.P = scan.shape
        self.bins = [np.flatnonzero(scan[c]) for c in range(self.ncls)]
        self.counts = [scan[c, b].astype(np.uint64) for c, b in enumerate(self.bins)]


def _finish(tot, q, norm, known, P, class_weights, regularization, through_double=False):
    """The reference's steps behind the sums (state_particle.cpp:117-120, 136-139, 154, 212).  through_double: the class sum
    rounded to double first and to float second — NOT the reference; what a test of a case's sensitivity compares with."""
    with np.errstate(all="ignore"):
        if round_to_f32(known) / f32(P) < 0.5:
            cost = f32(np.nan)
        else:
            cost = f32(0)
            for c, n in enumerate(tot):
                dot = f32(np.ldexp(float(n), -q)) if through_double else round_to_f32(n, q)
                cost = f32(float(cost) + float(dot) * 0.01 * float(f32(class_weights[c])))
            cost = f32(cost / round_to_f32(norm))
        return f32(1.0 / float(f32(cost + f32(regularization))))


def _particle(sc, q, dists, mask, src, fp, through_double=False, sums=None):
    """dists [ncls][P] / mask [P] (1 = unknown): the window; src[k]: the window cell scan bin k pairs with (None: k)."""
    known_cell = mask == 0
    tot, norm = [], 0
    for c in range(sc.ncls):
        at = sc.bins[c] if src is None else src[sc.bins[c]]
        vi = np.ldexp(dists[c, at].astype(np.float64), q)      # exact: a float64 holds a float times a power of two
        assert (vi == np.floor(vi)).all() and (vi < 2.0 ** 64).all()
        tot.append(exact_dot(sc.counts[c], vi.astype(np.uint64)))
        norm += int(sc.counts[c][known_cell[at]].sum(dtype=np.uint64))
    if sums is not None:
        sums.append((tot, norm))
    return _finish(tot, q, norm, int(known_cell.sum()), sc.P, fp.class_weights, fp.regularization, through_double)


def _centre(st):
    scale = f32(st["scale"])
    return f32(f32(st["dx_m"]) * scale + f32(st["init_x_px"])), f32(f32(st["dy_m"]) * scale + f32(st["init_y_px"])), scale


def weights_polar(oracle, class_maps, class_mask, resolution, tab, nb, nr, scan, res, fp, states, **kw):
    """Exact raw weights of a polar launch; states: STATE_DTYPE with have_init = 1; tab: oracle.polar_table.
    kw: sums = a list that receives (class totals * 2^Q, normalisation) of every particle scored; through_double."""
    om = oracle.OracleMap(class_maps, class_mask, resolution)
    q, sc = map_power(class_maps), Scan(scan)
    assert sc.P == nb * nr and states["have_init"].all()
    width, height = f32(om.cols) * f32(resolution), f32(om.rows) * f32(resolution)
    a, j = np.arange(nb * nr) % nb, np.arange(nb * nr) // nb
    w = np.zeros(len(states), f32)
    for p, st in enumerate(states):
        cx, cy, scale = _centre(st)
        if fp.force_on_map and (cx < 0 or cy < 0 or cx > width or cy > height):            # :163-168
            continue
        if fp.fixed_scale < 0 and (float(scale) < 10.0 ** float(f32(fp.scale_log_min)) or
                                   float(scale) > 10.0 ** float(f32(fp.scale_log_max))):   # :169-176
            continue
        dists, mask = oracle.local_map_polar(om, tab, cx, cy, scale, res)
        s = oracle.rot_shift(float(st["theta"]), nb)
        src = (a - s) % nb + nb * j                    # scan row a pairs with window row (a - s) mod nb (:129-142)
        w[p] = _particle(sc, q, dists, mask, src, fp, **kw)
    return w


def weights_cart(oracle, class_maps, class_mask, resolution, rows, cols, scan, res, fp, states, **kw):
    """Exact raw weights of a Cartesian launch (orc_compute_weights_cart: shift 0, no gates)."""
    om = oracle.OracleMap(class_maps, class_mask, resolution)
    q, sc = map_power(class_maps), Scan(scan)
    assert sc.P == rows * cols
    w = np.zeros(len(states), f32)
    for p, st in enumerate(states):
        cx, cy, scale = _centre(st)
        dists, mask = oracle.local_map_cart(om, cx, cy, float(st["theta"]), f32(res) * scale, rows, cols)
        w[p] = _particle(sc, q, dists, mask, None, fp, **kw)
    return w
