"""The 40-rotation heading search of StateParticle::computeWeight (src/state_particle.cpp:195-206) with every candidate's
cost formed EXACTLY — what the search kernels of csrc/tdr_score_init.hip are judged against.  CPU only; not a test module.

Per particle: the window from the oracle as it is (oracle.local_map_polar), the gates as np_oracle.compute_weights has them,
the candidates (theta_t, shift_t) from the reference's loop (:197: float t < 2 pi, double increment) and np_oracle.rot_shift.
A candidate's cost is

    cost64[t] = sum_c 0.01 * w_c * (sum count_c * d_c)  /  sum count_total * known

with scan row a paired with window row (a - shift_t) mod nb (:129-142).  Counts are whole numbers and a distance is a float,
i.e. an integer over 2^Q (int_exact_ref.map_power): both inner sums are formed in int64 (asserted not to overflow), the
weighted sum and the quotient as a Fraction, rounded to a double once.  The NaN rule of :117-120 (fewer than half of the
window's cells known) takes every candidate out; a zero denominator follows the reference's float division (x / 0 = inf,
0 / 0 = NaN): such a candidate never wins (:200-203, strict `<` against FLT_MAX).

Candidates that share a bin shift (nb < 40) have the same cost; the reference keeps the FIRST (:200-203).  check_choice
holds a search to that rule and to  cost64[chosen] <= min cost64 * (1 + TAU)."""
import math
from fractions import Fraction

import numpy as np

from int_exact_ref import map_power
from oracle import np_oracle

f32 = np.float32
TAU = 2e-5            # the project's near-tie figure (tests/test_gpu_fuzz.py, test_gpu_parity.py), here on the COST
FLT_MAX = f32(3.402823466e+38)
GATED, ALL_NAN, SEARCHED = 0, 1, 2


def candidates(nb):
    """[(theta_t float32, shift_t)] of the reference's loop."""
    out, t = [], f32(0)
    while float(t) < 2 * math.pi:
        out.append((t, np_oracle.rot_shift(t, nb)))
        t = f32(float(t) + 2 * math.pi / 40)
    return out


class Search:
    """The exact search of every particle of `states` (have_init == 1: kind GATED, not looked at).
    kind[p]; thetas [T] float32; shifts [T]; first[t]: t is the first candidate of its shift;
    cost64 [n][T] (inf: cannot win); best[p]: the first candidate of the cheapest shift class, -1 if none can win."""

    def __init__(self, oracle, class_maps, class_mask, resolution, tab, nb, nr, scan, res, fp, states):
        om = oracle.OracleMap(class_maps, class_mask, resolution)
        ncls = class_maps.shape[0]
        scan = np.asarray(scan, f32).reshape(ncls, nr, nb)
        assert (scan >= 0).all() and (scan == np.floor(scan)).all() and scan.sum() < 2.0 ** 22
        counts = scan.astype(np.int64)
        total = counts.sum(0)
        q = map_power(class_maps)
        assert float(np.max(class_maps, initial=0.0)) * 2.0 ** q * float(scan.sum()) < 2.0 ** 62, "int64 sums would overflow"
        cand = candidates(nb)
        self.thetas = np.asarray([t for t, _ in cand], f32)
        self.shifts = np.asarray([s for _, s in cand], np.int64)
        self.first = np.asarray([s not in self.shifts[:t] for t, s in enumerate(self.shifts)])
        cw = [Fraction(0.01 * float(f32(fp.class_weights[c]))) for c in range(ncls)]
        width, height = f32(om.cols) * f32(resolution), f32(om.rows) * f32(resolution)
        n, T, P = len(states), len(cand), nb * nr
        self.n, self.nb = n, nb
        self.kind = np.full(n, GATED, np.int64)
        self.cost64 = np.full((n, T), np.inf)
        self.best = np.full(n, -1, np.int64)
        distinct = sorted(set(int(s) for s in self.shifts))
        for p, st in enumerate(states):
            if st["have_init"]:
                continue
            scale = f32(st["scale"])
            cx = f32(f32(st["dx_m"]) * scale + f32(st["init_x_px"]))
            cy = f32(f32(st["dy_m"]) * scale + f32(st["init_y_px"]))
            if fp.force_on_map and (cx < 0 or cy < 0 or cx > width or cy > height):            # :163-168
                continue
            if fp.fixed_scale < 0 and (float(scale) < 10.0 ** float(f32(fp.scale_log_min)) or
                                       float(scale) > 10.0 ** float(f32(fp.scale_log_max))):   # :169-176
                continue
            dists, mask = oracle.local_map_polar(om, tab, cx, cy, scale, res)
            known = (mask == 0).reshape(nr, nb)
            if f32(f32(known.sum()) / f32(P)) < 0.5:                                           # :117-120
                self.kind[p] = ALL_NAN
                continue
            self.kind[p] = SEARCHED
            di = np.ldexp(dists.astype(np.float64), q)             # exact: a double holds a float times a power of two
            assert (di == np.floor(di)).all()
            di = di.astype(np.int64).reshape(ncls, nr, nb)
            ki = known.astype(np.int64)
            by_shift = {}
            for s in distinct:
                num = sum((cw[c] * int((counts[c] * np.roll(di[c], s, axis=1)).sum()) for c in range(ncls)), Fraction(0))
                den = int((total * np.roll(ki, s, axis=1)).sum())
                # (the numerator carries 2^q; a zero denominator: inf or NaN in the reference, never below FLT_MAX)
                by_shift[s] = float(num / den) / 2.0 ** q if den > 0 else np.inf
                if den > 0 and not by_shift[s] < float(FLT_MAX):
                    by_shift[s] = np.inf
            self.cost64[p] = [by_shift[int(s)] for s in self.shifts]
            if np.isfinite(self.cost64[p]).any():
                self.best[p] = int(np.argmin(self.cost64[p]))      # (argmin: the first of equal values)
            else:
                self.kind[p] = ALL_NAN

    def searched(self):
        return np.flatnonzero(self.kind == SEARCHED)

    def separated(self, tau=TAU):
        """Per searched particle: is the cheapest shift class below every other by more than tau (relative)?"""
        out = []
        for p in self.searched():
            c = self.cost64[p][self.first]
            lo = c.min()
            rest = np.delete(c, int(np.argmin(c)))
            out.append(bool(len(rest) == 0 or rest.min() > lo * (1 + tau)))
        return np.asarray(out, bool)

    def wanted_batches(self):
        """64-particle batches (identity order) in which the search has something to do: the others return early."""
        want = self.kind != GATED
        return int(sum(want[b:b + 64].any() for b in range(0, self.n, 64)))


def check_choice(search, theta_before, theta, have_init, raw, raw_oracle, have_init_before, tau=TAU, only=None):
    """Asserts the rules of the module's docstring on a search's result; returns the largest excess
    cost64[chosen] / min cost64 - 1 over the searched particles (0 if the best class was chosen everywhere).
    raw_oracle: the oracle's weights for the same un-initialised states (what gated and all-NaN particles must carry).
    only: the particles to look at (default: all)."""
    worst = 0.0
    for p in (range(search.n) if only is None else only):
        kind = search.kind[p]
        if kind == GATED:
            assert have_init[p] == have_init_before[p], f"particle {p}: have_init of an untouched particle moved"
            assert theta[p].tobytes() == theta_before[p].tobytes(), f"particle {p}: theta of an untouched particle moved"
            if not have_init_before[p]:
                assert raw[p].tobytes() == raw_oracle[p].tobytes(), (p, raw[p], raw_oracle[p])
            continue
        assert have_init[p] == 1, f"particle {p} was not initialised"
        if kind == ALL_NAN:
            assert theta[p] == 0, f"particle {p}: no candidate can win, theta must stay 0, is {theta[p]}"
            assert raw[p].tobytes() == raw_oracle[p].tobytes(), (p, raw[p], raw_oracle[p])
            continue
        hit = np.flatnonzero(search.thetas.view(np.uint32) == theta[p:p + 1].view(np.uint32)[0])
        assert len(hit) == 1, f"particle {p}: theta {theta[p]!r} is none of the candidates"
        t = int(hit[0])
        assert search.first[t], (f"particle {p}: candidate {t} (shift {search.shifts[t]}) is not the first of its shift class "
                                 f"({int(np.flatnonzero(search.shifts == search.shifts[t])[0])} is)")
        lo = search.cost64[p].min()
        c = search.cost64[p][t]
        assert c <= lo * (1 + tau), (f"particle {p}: cost {c!r} of the chosen candidate {t} exceeds the minimum {lo!r} "
                                     f"(candidate {search.best[p]}) by {c / lo - 1:.3e} > {tau}")
        if c > lo:
            worst = max(worst, c / lo - 1)
    return worst
