"""Hand-worked particles for the KLD-sampling count and the bins they fall in (not a test module): tests/test_kld_ref.py
holds the restatement to them, tests/test_kld.py the kernel.  Every expectation below is worked out in its comment, none
comes from running the code."""
import math

import numpy as np

from top_down_renderer_amd.synth import STATE_DTYPE

F32 = np.float32
PI = math.pi


def state(cx=0.0, cy=0.0, theta=0.0, scale=1.0, have_init=1, dx=0.0, dy=0.0):
    """One State whose centre is (dx * scale + cx, dy * scale + cy)."""
    s = np.zeros(1, STATE_DTYPE)
    s["init_x_px"], s["init_y_px"], s["dx_m"], s["dy_m"] = F32(cx), F32(cy), F32(dx), F32(dy)
    s["theta"], s["scale"], s["have_init"] = F32(theta), F32(scale), have_init
    return s


def states(rows):
    return np.concatenate([state(**r) for r in rows]) if rows else np.zeros(0, STATE_DTYPE)


# position, bin edge 4 px (a power of two: the IEEE quotient is exact): (centre, bin)
POS_BIN4 = [
    (-0.5, -1),                                    # -0.125 -> floor -1 (truncation would say 0)
    (0.0, 0),
    (-0.0, 0),                                     # floor(-0) = -0 -> 0
    (12.0, 3),                                     # exactly on the edge 3 * bin: belongs to the bin it opens
    (float(np.nextafter(F32(12), F32(0))), 2),     # one ulp below it
    (-4.0, -1),                                    # on a negative edge
    (float(np.nextafter(F32(-4), F32(-5))), -2),
    (2097148.0, 524287),                           # 524287 * 4: the last bin's lower edge
    (2097152.0, 524287),                           # 2^19 bins: clamped into the last one
    (1e9, 524287),
    (-2097152.0, -524288),                         # -2^19 * 4: the first bin's lower edge
    (-2097156.0, -524288),                         # one bin further out: clamped
    (-1e9, -524288),
]
# a centre that needs the product: dx * s + init = 2.5 * 2 + 7 = 12 -> bin 3; 2.5 * 2 - 5.5 = -0.5 -> bin -1
POS_PRODUCT = [(dict(dx=2.5, scale=2.0, cx=7.0, dy=2.5, cy=-5.5), (3, -1))]

# heading: v = float(theta) * T / 2 / pi, rounded half away from zero, then mod T (floor mod)
#   float32(pi) = 3.14159274 is ABOVE pi by 2.8e-8 relative, float32(5 pi) = 15.70796299 is BELOW 5 pi by 1.8e-8 relative
HEADING = {
    1: [(0.0, 0), (PI, 0), (-PI, 0), (5 * PI, 0), (-7.3, 0)],       # one bin: everything mod 1
    36: [(0.0, 0),
         (PI, 18),            # v = 18.00000005 -> 18
         (-PI, 18),           # v = -18.00000005 -> -18 -> 18: the two sides of the cut share a bin
         (5 * PI, 18),        # v = 90.000003 -> 90 = 2 * 36 + 18: whole turns drop out
         (-7.3, 30)],         # v = -7.3 * 36 / 6.2832 = -41.83 -> -42 -> -42 + 72 = 30
    511: [(0.0, 0),
          (PI, 256),          # v = 255.5 * (1 + 2.8e-8) = 255.5000057: above the tie -> 256
          (-PI, 255),         # v = -255.5000057 -> -256 -> 255
          (5 * PI, 255),      # v = 1277.5 * (1 - 1.8e-8) = 1277.49997: below the tie -> 1277 = 2 * 511 + 255
          (-7.3, 428)],       # v = -7.3 * 511 / 6.2832 = -593.70 -> -594 -> -594 + 1022 = 428
}

# scale: bits >> (23 - b).  1.0 = 0x3F800000, 1.5 = 0x3FC00000, 2.0 = 0x40000000, nextafter(2, 0) = 0x3FFFFFFF
SCALE = {
    0: [(1.0, 0x7F), (1.5, 0x7F), (2.0, 0x80), (float(np.nextafter(F32(2), F32(0))), 0x7F)],          # the exponent alone
    1: [(1.0, 0xFE), (1.5, 0xFF), (2.0, 0x100), (float(np.nextafter(F32(2), F32(0))), 0xFF)],         # halves of an octave
    6: [(1.0, 0x1FC0), (1.5, 0x1FE0), (2.0, 0x2000), (float(np.nextafter(F32(2), F32(0))), 0x1FFF)],  # 64 bins an octave
}

# particles without a key: a non-finite centre or scale, a scale that is not positive
NO_KEY_ROWS = [dict(cx=math.nan), dict(cy=math.inf), dict(cx=-math.inf), dict(scale=math.nan), dict(scale=math.inf),
               dict(scale=0.0), dict(scale=-1.0), dict(dx=math.nan), dict(dy=math.inf, scale=2.0)]


def pack(ix, iy, it, isc):
    return (ix + 524288) << 43 | (iy + 524288) << 23 | it << 14 | isc


def hand_set():
    """(states, expected keys as Python ints or None) over all of the above, for T = 36, b = 3, bin 4: scale 1 -> bits >> 20 =
    0x3F8, scale 2 -> 0x400."""
    rows, want = [], []
    for c, b in POS_BIN4:
        rows += [dict(cx=c), dict(cy=c)]
        want += [pack(b, 0, 0, 0x3F8), pack(0, b, 0, 0x3F8)]
    for kw, (bx, by) in POS_PRODUCT:
        rows.append(kw)
        want.append(pack(bx, by, 0, 0x400))
    for th, b in HEADING[36]:
        rows.append(dict(theta=th))
        want.append(pack(0, 0, b, 0x3F8))
    rows.append(dict(theta=1.0, have_init=0))       # no heading: bin T
    want.append(pack(0, 0, 36, 0x3F8))
    for kw in NO_KEY_ROWS:
        rows.append(kw)
        want.append(None)
    return states(rows), want
