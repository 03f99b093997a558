"""What the pose statistics (tdr_k_mean_cov: meanLikelihood, computeMeanCov, computeCov, the geometric-mean scale of
freezeScale) must give at any particle count (shared by tests/test_pose_ref.py and tests/test_pose_stats.py; not a test
module).

The kernels sum in double, in an order of their own; the CPU oracle restates the reference's serial float32 sums, which
drift by pixels at the particle counts in use (`float_chain_drift` below).  So this reference keeps the two apart:

  * every PER-PARTICLE float32 expression is the kernel's, rounding for rounding: x = f32(f32(dx * sc) + init_x) (the
    library is built without contraction: two roundings), cos / sin from the library's host restatement of the host
    libm's cosf / sinf (tests/test_libm.py pins the device functions to them bit for bit), d = f32(v - ref), the heading
    wrap `while d > pi: d = f32(f64(d) - 2 pi)` and its mirror, the products f32(d[a] * d[b]);
  * every SUM is exact: math.fsum over the float64-widened terms;
  * then the kernel's last steps: f32(tot) / f32(n), atan2 of the two float ratios, f32(ct) / f32(n - 1),
    f32(exp(fsum(log(f64 sc)) / n)).

Nothing here imports the package's kernels; the sin / cos helper is host code of the library."""
import ctypes as C
import math

import numpy as np

F32 = np.float32
PAIRS = [(a, b) for a in range(4) for b in range(a, 4)]        # the kernel's order of the ten second moments
FIELDS = ("init_x_px", "init_y_px", "dx_m", "dy_m", "theta", "scale")
# the two shapes of the reduction (csrc/tdr_filter_dev.h): one workgroup of 1024 threads up to 4096 particles, above that
# 128 workgroups of 256 threads
SINGLE_MAX_N, SINGLE_THREADS, MC_WGS, MC_THREADS = 4096, 1024, 128, 256
# double additions a sum passes through at 2 000 003 particles: 62 per thread, 6 shuffle steps, 4 waves, 128 workgroups
# = 200 < 256 (fewer at every smaller size and on the one-workgroup path: 4 + 6 + 16)
SUM_STEPS = 256


def planes(st):
    """The six float planes {init_x, init_y, dx, dy, theta, scale} of a STATE_DTYPE array, or of a [>= 6][n] float32
    array in the device's plane order."""
    if getattr(st, "dtype", None) is not None and st.dtype.names:
        return [np.ascontiguousarray(st[f], F32) for f in FIELDS]
    return [np.ascontiguousarray(st[i], F32) for i in range(6)]


def sincos(theta):
    """The host libm's sinf / cosf as the library restates them (the variant this host's libm takes)."""
    from top_down_renderer_amd import _lib
    L = _lib.load()
    v = L.tdr_libm_variant()
    assert v in (0, 1)
    x = np.ascontiguousarray(theta, F32)
    s, c = np.empty_like(x), np.empty_like(x)
    assert L.tdr_sincosf_host(x.ctypes.data_as(C.c_void_p), len(x), v, s.ctypes.data_as(C.c_void_p),
                              c.ctypes.data_as(C.c_void_p)) == 0
    return s, c


def ml_states(st):
    """mlState of every particle (state_particle.cpp:98-102) in the kernel's float32: (x, y, theta, scale)."""
    ix, iy, dx, dy, th, sc = planes(st)
    x = (dx * sc).astype(F32) + ix          # float32 arrays: NumPy rounds the product, then the sum
    y = (dy * sc).astype(F32) + iy
    return x.astype(F32), y.astype(F32), th, sc


def first_terms(st):
    """The seven per-particle terms of the first pass, widened to float64: x, y, theta, scale, cos, sin, log scale."""
    x, y, th, sc = ml_states(st)
    s, c = sincos(th)
    with np.errstate(all="ignore"):
        lg = np.log(sc.astype(np.float64))
    return [v.astype(np.float64) for v in (x, y, th, sc, c, s)] + [lg]


def wrap(d):
    """`while (d > M_PI) d = (float)((double)d - 2 * M_PI)` and the mirror, on a float32 array."""
    d = d.astype(F32).copy()
    while True:
        hi = d.astype(np.float64) > math.pi
        if not hi.any():
            break
        d[hi] = (d[hi].astype(np.float64) - 2 * math.pi).astype(F32)
    while True:
        lo = d.astype(np.float64) < -math.pi
        if not lo.any():
            break
        d[lo] = (d[lo].astype(np.float64) + 2 * math.pi).astype(F32)
    return d


def second_terms(st, about):
    """The ten per-particle products f32(d[a] * d[b]) about the float32 point `about`, widened to float64 (PAIRS order)."""
    about = np.asarray(about, F32)
    x, y, th, sc = ml_states(st)
    d = [(x - about[0]).astype(F32), (y - about[1]).astype(F32), wrap((th - about[2]).astype(F32)),
         (sc - about[3]).astype(F32)]
    return [(d[a] * d[b]).astype(F32).astype(np.float64) for a, b in PAIRS]


def exact(term):
    return math.fsum(term.tolist())


def finish_mean(tot, n):
    """mean[4] and the geometric-mean scale from the seven totals (float64), the kernel's last steps."""
    fn = F32(n)
    with np.errstate(all="ignore"):
        mean = np.array([F32(tot[0]) / fn, F32(tot[1]) / fn, np.arctan2(F32(tot[5]) / fn, F32(tot[4]) / fn),
                         F32(tot[3]) / fn], F32)
        geo = F32(math.exp(tot[6] / n)) if math.isfinite(tot[6]) else F32(np.exp(np.float64(tot[6]) / n))
    return mean, geo


def finish_cov(ct, n):
    """cov[4][4] from the ten totals: f32(ct) / f32(n - 1), mirrored."""
    cov = np.zeros((4, 4), F32)
    with np.errstate(all="ignore"):
        for (a, b), t in zip(PAIRS, ct):
            cov[a, b] = cov[b, a] = F32(t) / F32(n - 1)
    return cov


def mean_ref(st):
    """(mean[4] float32, geometric-mean scale float32, the seven exact totals)."""
    terms = first_terms(st)
    n = len(terms[0])
    tot = [exact(t) for t in terms]
    mean, geo = finish_mean(tot, n)
    return mean, geo, tot


def cov_ref(st, about):
    """(cov[4][4] float32 about `about`, absum[4][4] = the sum of |term| of each entry, the ten exact totals)."""
    terms = second_terms(st, about)
    n = len(terms[0])
    ct = [exact(t) for t in terms]
    absum = np.zeros((4, 4))
    for (a, b), t in zip(PAIRS, terms):
        absum[a, b] = absum[b, a] = exact(np.abs(t))
    return finish_cov(ct, n), absum, ct


# ---- tolerances (derived; "ulp" = the float32 spacing at the reference value) ------------------------------------------------
def ulp(v):
    return np.spacing(np.abs(np.asarray(v, F32))).astype(np.float64)


MEAN_ULPS = 2          # the double sum is within << half an ulp of the exact one; the float cast may land on the other side
#                        of a tie, and the division keeps that to one more ulp
HEADING_TOL = 1e-6     # atan2f's inputs within 2 ulp each, resultant length >= 0.5, one float rounding near pi is 2.4e-7
GEO_ULPS = 2


def cov_tol(cov, absum, n):
    """2 ulp(ref) + SUM_STEPS * 2^-53 * sum|term| / (n - 1), per entry."""
    return MEAN_ULPS * ulp(cov) + SUM_STEPS * 2.0 ** -53 * absum / max(n - 1, 1)


# ---- the kernel's own order of summation, in NumPy ---------------------------------------------------------------------------
def kernel_order_sum(term):
    """The float64 sum of `term` in the order tdr_k_mean_cov adds it up: strided per-thread serial sums, the 64-lane
    shuffle tree, the waves of a workgroup in order, the workgroups in order."""
    n = len(term)
    wgs, threads = (1, SINGLE_THREADS) if n <= SINGLE_MAX_N else (MC_WGS, MC_THREADS)
    step = wgs * threads
    rows = -(-n // step)
    padded = np.zeros(rows * step)
    padded[:n] = term
    acc = np.zeros(step)
    with np.errstate(all="ignore"):
        for r in padded.reshape(rows, step):
            acc = acc + r                              # thread t: particles t, t + step, ... one after the other
        v = acc.reshape(-1, 64)                        # waves
        for o in (32, 16, 8, 4, 2, 1):                 # v += __shfl_down(v, o): lanes past the end read themselves
            nxt = v + v
            nxt[:, :64 - o] = v[:, :64 - o] + v[:, o:]
            v = nxt
        waves = v[:, 0].reshape(wgs, threads // 64)
        total = 0.0
        for g in range(wgs):
            t = 0.0
            for w in range(threads // 64):
                t = t + waves[g, w]
            total = total + t
    return float(total)


def kernel_order(st, about=None):
    """The 24 result floats as the kernel's order of float64 additions gives them (NumPy's log / exp / arctan2 stand in for
    the device's)."""
    terms = first_terms(st)
    n = len(terms[0])
    mean, geo = finish_mean([kernel_order_sum(t) for t in terms], n)
    ref = mean if about is None else np.asarray(about, F32)
    cov = finish_cov([kernel_order_sum(t) for t in second_terms(st, ref)], n)
    out = np.zeros(24, F32)
    out[:4], out[4:20], out[20] = mean, cov.reshape(-1), geo
    return out


# ---- the reference's float32 chain ---------------------------------------------------------------------------------------
def float_chain(st):
    """meanLikelihood + computeMeanCov with the reference's serial float32 accumulators (np.cumsum in float32 is that
    chain): (mean[4], cov[4][4]).  What the kernels deliberately leave; see float_chain_drift."""
    x, y, th, sc = ml_states(st)
    s, c = sincos(th)
    n = len(x)

    def chain(v):
        return np.cumsum(v.astype(F32), dtype=F32)[-1]
    fn = F32(n)
    mean = np.array([chain(x) / fn, chain(y) / fn, np.arctan2(chain(s) / fn, chain(c) / fn), chain(sc) / fn], F32)
    d = [(x - mean[0]).astype(F32), (y - mean[1]).astype(F32), wrap((th - mean[2]).astype(F32)), (sc - mean[3]).astype(F32)]
    cov = np.zeros((4, 4), F32)
    for a, b in PAIRS:
        cov[a, b] = cov[b, a] = chain((d[a] * d[b]).astype(F32)) / F32(n - 1)
    return mean, cov


def float_chain_drift(st):
    """How far the float32 chain is from the exact sums on `st`: (|mean x error| in px, relative error of cov(0,0),
    relative error of cov(3,3))."""
    mean, cov = float_chain(st)
    m, _, _ = mean_ref(st)
    c, _, _ = cov_ref(st, m)
    return (abs(float(mean[0]) - float(m[0])), abs(float(cov[0, 0]) - float(c[0, 0])) / float(c[0, 0]),
            abs(float(cov[3, 3]) - float(c[3, 3])) / float(c[3, 3]))


# ---- the inputs of the GPU tests -----------------------------------------------------------------------------------------
SIZES = (1, 2, 3, 63, 1024, 1025, 4095, 4096, 4097, 32_767, 32_768, 32_769, 100_003, 2_000_003)
LARGE = 100_003                      # from here on only the mixed family ("turns") runs
FAMILIES = ("cluster", "turns", "one_scale")
SENTINELS = (0, -1, 4095, 4096, 32_767, 32_768)
ONE_SCALE = F32(2.7182817)
STATE_DTYPE = np.dtype([("init_x_px", "<f4"), ("init_y_px", "<f4"), ("dx_m", "<f4"), ("dy_m", "<f4"), ("theta", "<f4"),
                        ("scale", "<f4"), ("have_init", "u1"), ("pad", "u1", (3,))])


def sentinels(n):
    return sorted({(s + n) % n for s in SENTINELS if -n <= s < n})


def make_states(n, family, seed=None):
    """n particles like a converged filter (seeded): x ~ 2000 +- 3 px, y ~ 1500 +- 3 px, headings around 3.1 rad kept in (-pi, pi] —
    the mean sits at the +-pi cut and three differences in ten wrap once — and
      cluster    scales lognormal over [0.5, 10];
      turns      the same with whole turns added to the headings (theta + 2 pi k, k in [-3, 3]): the wrap loop runs
                 several times; |theta| stays below 64;
      one_scale  every scale the one float ONE_SCALE (a frozen filter).
    The sentinel particles (indices 0, n-1, 4095, 4096, 32 767, 32 768 where n has them) stand 200 px and more off in
    init_x and, but for one_scale, carry a scale of their own."""
    rng = np.random.default_rng(1000 * SIZES.index(n) + FAMILIES.index(family) if seed is None else seed)
    st = np.zeros(n, STATE_DTYPE)
    st["have_init"] = 1
    sc = np.clip(np.exp(rng.normal(0.8, 0.6, n)), 0.5, 10.0).astype(F32)
    if family == "one_scale":
        sc[:] = ONE_SCALE
    st["scale"] = sc
    st["dx_m"] = rng.normal(0, 1.5, n).astype(F32)
    st["dy_m"] = rng.normal(0, 1.5, n).astype(F32)
    # the pixel position is what clusters: init = target - dx * scale
    st["init_x_px"] = (2000.0 + rng.normal(0, 3, n) - st["dx_m"].astype(np.float64) * sc).astype(F32)
    st["init_y_px"] = (1500.0 + rng.normal(0, 3, n) - st["dy_m"].astype(np.float64) * sc).astype(F32)
    th = 3.1 + rng.normal(0, 0.08, n)
    th = np.where(th > math.pi, th - 2 * math.pi, th)       # stored in (-pi, pi]: three in ten sit across the cut
    if family == "turns":
        th = th + 2 * math.pi * rng.integers(-3, 4, n)
    st["theta"] = th.astype(F32)
    for j, i in enumerate(sentinels(n)):
        st["init_x_px"][i] += F32(200.0 + 16.0 * j)
        if family != "one_scale":
            st["scale"][i] = F32(30.0 + j)
    assert float(np.abs(st["theta"]).max()) <= 64.0
    s, c = np.sin(st["theta"].astype(np.float64)), np.cos(st["theta"].astype(np.float64))
    assert math.hypot(s.mean(), c.mean()) >= 0.5            # a well-conditioned mean heading
    return st


def far_about(st):
    """The mlState of a particle whose heading is several turns away from the cluster (computeCov's reference point)."""
    x, y, th, sc = ml_states(st[:1])
    return np.array([x[0] + F32(1.5), y[0] - F32(2.25), F32(float(th[0]) % (2 * math.pi) - 4 * 2 * math.pi), sc[0]], F32)


def to_planes(st, cap):
    """[7][cap] float32 in the device's plane order, the padding [n, cap) of every plane NaN."""
    n = len(st)
    out = np.full((7, cap), np.nan, F32)
    for i, f in enumerate(FIELDS):
        out[i, :n] = st[f]
    out[6, :n] = st["have_init"]
    return out


# ---- the reference of one (n, family) input, computed once, and the comparison every test makes ------------------------------
class Ref:
    """The input `make_states(n, family)` and its exact reference; the covariance about a point is computed on demand and
    kept (the GPU tests pass the mean the device returned, which is the reference's own bits whenever it is right)."""
    _made = {}

    def __init__(self, n, family):
        self.n, self.family = n, family
        self.st = make_states(n, family)
        self.mean, self.geo, self.tot = mean_ref(self.st)
        self.about = far_about(self.st)
        self._cov = {}

    @classmethod
    def get(cls, n, family):
        if (n, family) not in cls._made:
            cls._made[(n, family)] = cls(n, family)
        return cls._made[(n, family)]

    def cov(self, about):
        key = np.asarray(about, F32).tobytes()
        if key not in self._cov:
            self._cov[key] = cov_ref(self.st, about)
        return self._cov[key]


def check_means(out, ref):
    """The mean, heading and geometric-mean part of 24 result floats against `ref`; returns the deviations as fractions of
    their tolerances {"means", "heading", "geo"} after asserting them."""
    out = np.asarray(out, F32)
    dev = {}
    m = [0, 1, 3]
    err = np.abs(out[m].astype(np.float64) - ref.mean[m].astype(np.float64)) / ulp(ref.mean[m])
    dev["means"] = float(err.max())
    assert dev["means"] <= MEAN_ULPS, f"mean x / y / scale {out[m]} vs {ref.mean[m]}: {err} ulp"
    dh = abs((float(out[2]) - float(ref.mean[2]) + math.pi) % (2 * math.pi) - math.pi)
    dev["heading"] = dh
    assert dh <= HEADING_TOL, f"mean heading {out[2]!r} vs {ref.mean[2]!r}: {dh:.3e} rad"
    assert -math.pi <= float(out[2]) <= math.pi
    dev["geo"] = abs(float(out[20]) - float(ref.geo)) / float(ulp(ref.geo))
    assert dev["geo"] <= GEO_ULPS, f"geometric-mean scale {out[20]!r} vs {ref.geo!r}: {dev['geo']} ulp"
    assert not out[21:24].any() and not np.signbit(out[21:24]).any()
    return dev


def check_cov(out, ref, about):
    """The 16 covariance floats of `out` against the exact covariance about the float32 point `about`: the derived bound
    where the reference is finite, the same non-finite value where it is not (n = 1 divides by zero), symmetry in bits.
    Returns the largest deviation as a fraction of the bound."""
    got = np.asarray(out, F32)[4:20].reshape(4, 4)
    assert np.array_equal(got.view(np.uint32), got.T.view(np.uint32)), "covariance is not symmetric bit for bit"
    cov, absum, _ = ref.cov(about)
    fin = np.isfinite(cov)
    assert np.array_equal(np.isfinite(got), fin), f"finite entries differ:\n{got}\nvs\n{cov}"
    assert np.array_equal(got[~fin], cov[~fin], equal_nan=True), f"non-finite entries differ:\n{got}\nvs\n{cov}"
    if not fin.any():
        return 0.0
    tol = cov_tol(cov, absum, ref.n)
    ratio = np.abs(got.astype(np.float64) - cov.astype(np.float64))[fin] / tol[fin]
    assert ratio.max() <= 1.0, f"covariance about {about}:\n{got}\nvs\n{cov}\n|difference| / bound:\n{ratio}"
    return float(ratio.max())


def sentinel_effect(ref, i):
    """How far the asserted outputs move, in units of their tolerances, when particle i's terms are missing from the sums
    (a dropped partial sum, an off-by-one at a stride end): the largest over the means, the geometric mean and the
    covariance about the mean and about `ref.about`.  n stays: a kernel that skips a particle still divides by n."""
    one = ref.st[i:i + 1]
    first = [float(t[0]) for t in first_terms(one)]
    mean, geo = finish_mean([t - f for t, f in zip(ref.tot, first)], ref.n)
    m = [0, 1, 3]
    moved = [float((np.abs(mean[m].astype(np.float64) - ref.mean[m]) / (MEAN_ULPS * ulp(ref.mean[m]))).max()),
             abs(float(mean[2]) - float(ref.mean[2])) / HEADING_TOL,
             abs(float(geo) - float(ref.geo)) / (GEO_ULPS * float(ulp(ref.geo)))]
    for about in (ref.mean, ref.about):
        cov, absum, ct = ref.cov(about)
        second = [float(t[0]) for t in second_terms(one, about)]
        less = finish_cov([t - s for t, s in zip(ct, second)], ref.n)
        with np.errstate(all="ignore"):
            r = np.abs(less.astype(np.float64) - cov.astype(np.float64)) / cov_tol(cov, absum, ref.n)
        if np.isfinite(r).any():
            moved.append(float(np.nanmax(np.where(np.isfinite(r), r, np.nan))))
    return max(moved)
