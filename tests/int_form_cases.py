"""The launches of tests/test_int_form_limits.py (GPU) and of check (b) of tests/test_int_exact_ref.py (CPU): scans, maps and
particles at the magnitude limits the integer form of a scoring launch sets itself.  Not a test module.

A count per bin below 2^24; a single class below 4096 in the descriptor, everything else on the list; the Cartesian block
descriptor's 24 count bits; the bound on the scan's total count ("mass bound", int_form_off) below 2^24; dictionary values
with value * 2^q below 2^32; 64-bit class sums.  `form` is what the launch must run in: "integer" (the weights are the exact
reference's bits) or "float" (the device notices, the float kernel does the launch).  int_form_expected() restates the
device's rules on the host; tests/test_int_exact_ref.py holds the table against it."""
import numpy as np

from top_down_renderer_amd import synth

import int_exact_ref

NCLS = 6
TOP = 2 ** 24 - 1
LADDER = (1, 4095, 4096, 4097, 65535, 65536, TOP)
N_PARTICLES = 256
DICT_TOP = np.float32(512.0 - 2.0 ** -14)      # * 2^23 = 2^32 - 2^9: the largest dictionary integer with q = 23 is just below 2^32
DICT_VALUES = (np.float32(2.0 ** -23), np.float32(0.5), np.float32(1.5), np.float32(3.25))

# name -> (form, scan, map, polar (nb, nr), Cartesian (rows, cols)); map: "scene" = distance maps min(50, sqrt(d2)), q = 23
TABLE = {
    "ladder": ("integer", "ladder", "scene", (64, 24), (64, 24)),
    "ladder_one_bin_2p24": ("float", "ladder_2p24", "scene", (64, 24), (64, 24)),
    "several_classes": ("integer", "multi", "scene", (48, 20), (48, 24)),
    "several_classes_sum_2p24": ("float", "multi_sum", "scene", (48, 20), (48, 24)),
    "every_bin_listed": ("integer", "all_listed", "scene", (32, 16), (32, 16)),
    "class_sum_past_2p53": ("integer", "past_2p53", "scene", (48, 20), (48, 24)),
    "dictionary_below_2p32": ("integer", "mass_below", "dict_edge", (48, 20), (48, 24)),
    "dictionary_at_2p32": ("float", "ladder", "dict_over", (48, 20), (48, 24)),
    "mass_bound_2p24_minus_1": ("integer", "mass_below", "scene", (48, 20), (48, 24)),
    "mass_bound_2p24": ("float", "mass_at", "scene", (48, 20), (48, 24)),
    "mass_bound_wraps": ("float", "wrap", "scene", (256, 256), (256, 256)),
}
NAMES = tuple(TABLE)
KINDS = ("polar", "cart")


def mass_bound(scan):
    """The prep kernels' bound on (total count) / 256: sum over the bins with 1 <= sum < 2^24 of (sum >> 8) + 1."""
    s = np.asarray(scan, np.float64).sum(axis=0)
    s = s[(s >= 1) & (s < 2 ** 24)].astype(np.int64)
    return int(((s >> 8) + 1).sum())


def int_form_expected(scan, class_maps):
    """The device's own rules for the integer form, on the host."""
    scan = np.asarray(scan, np.float64)
    sums = scan.sum(axis=0)
    whole = bool((scan >= 0).all() and (scan == np.floor(scan)).all() and (scan < 2 ** 24).all() and (sums < 2 ** 24).all())
    q = int_exact_ref.map_power(class_maps)
    dict_ok = float(np.max(class_maps)) * 2.0 ** q < 2.0 ** 32 and len(np.unique(class_maps)) <= 1024
    return whole and dict_ok and mass_bound(scan) < 2 ** 24


# ---- scans: [NCLS][P], one builder per name -----------------------------------------------------------------------------
def _ladder(rng, P):
    scan = np.zeros((NCLS, P), np.float32)
    bins = rng.permutation(P)[:P // 3]
    scan[rng.integers(0, NCLS, len(bins)), bins] = np.resize(np.asarray(LADDER, np.float32), len(bins))
    return scan, bins


def _multi(rng, P):
    scan = np.zeros((NCLS, P), np.float32)
    bins = rng.permutation(P)
    for b in bins[:40]:                                  # three classes, each in the millions: the list / the FULL codes
        scan[rng.permutation(NCLS)[:3], b] = rng.integers(1, 5_000_000, 3)
    scan[:, bins[40]] = TOP // NCLS                      # every class, the bin's sum 2^24 - 4
    scan[rng.integers(0, NCLS, 100), bins[41:141]] = rng.integers(1, 4, 100)
    return scan, bins


def _mass_below(rng, P, cls=0):
    """255 bins of 2^24 - 1 and one of 65534 * 256: the bound is 255 * 65536 + 65535 = 2^24 - 1, the total count 2^32 - 767"""
    scan = np.zeros((NCLS, P), np.float32)
    bins = rng.permutation(P)
    scan[cls, bins[:255]] = TOP
    scan[cls, bins[255]] = 65534 * 256
    return scan, bins


def make_scan(name, rng, P):
    if name == "ladder":
        return _ladder(rng, P)[0]
    if name == "ladder_2p24":
        scan, bins = _ladder(rng, P)
        scan[:, bins[0]] = 0
        scan[2, bins[0]] = 2.0 ** 24
        return scan
    if name == "multi":
        return _multi(rng, P)[0]
    if name == "multi_sum":                              # every class below 2^24, the bin's sum 18 000 000
        scan, bins = _multi(rng, P)
        scan[:, bins[3]] = 0
        scan[(1, 4), bins[3]] = 9_000_000
        return scan
    if name == "all_listed":                             # two classes of at least 4096 in EVERY bin: P entries on every list
        scan = np.zeros((NCLS, P), np.float32)
        c1 = rng.integers(0, NCLS, P)
        c2 = (c1 + 1 + rng.integers(0, NCLS - 1, P)) % NCLS
        scan[c1, np.arange(P)] = rng.integers(4096, 8192, P)
        scan[c2, np.arange(P)] = rng.integers(4096, 8192, P)
        return scan
    if name == "mass_below":
        return _mass_below(rng, P)[0]
    if name == "mass_at":                                # one more count of 1: the bound is 2^24, the total still below 2^32
        scan, bins = _mass_below(rng, P)
        scan[3, bins[256]] = 1
        return scan
    if name == "wrap":                                   # every bin adds 65 536 to the bound: 65 536 bins make 2^32
        scan = np.zeros((NCLS, P), np.float32)
        scan[rng.integers(0, NCLS, P), np.arange(P)] = rng.integers(16_776_960, 16_777_216, P)
        return scan
    raise KeyError(name)


def _past_2p53(oracle, case, rng):
    """One class alone, counts in the millions: every particle's class total lies past 2^53.  For particle 0 the total is
    MADE: T = H 2^31 + 2^30 + 1 with H even, 2^23 <= H < 2^24.  T lies just above the middle of two floats, so it rounds UP;
    rounded to double first (a unit of 4 at 2^54) the 1 is lost, the middle is hit and ties-to-even rounds DOWN.  The bins
    are those where particle 0's window holds a whole distance d >= 16 (V = d 2^23), 1 (V = 2^23) and sqrt 2 (V odd) in that
    class: the count at sqrt 2 from T mod 2^23, the rest spread over the far bins and the bin at 1."""
    P = case["P"]
    dists, mask, src = window_of(oracle, case, case["states"][0])
    v_odd = int(np.float32(np.sqrt(2.0)).view(np.uint32) & 0x7FFFFF | 0x800000)    # sqrt 2 = v_odd 2^-23
    assert v_odd & 1
    def build(H):
        T = (H << 31) + (1 << 30) + 1
        c_odd = (T * pow(v_odd, -1, 2 ** 23)) % 2 ** 23
        rest = (T - c_odd * v_odd) >> 23
        assert (rest << 23) + c_odd * v_odd == T
        for cls in range(NCLS):
            d = np.where(mask[src] == 0, dists[cls, src], 0)
            one, odd = np.flatnonzero(d == 1), np.flatnonzero(d == np.float32(np.sqrt(2.0)))
            far = np.flatnonzero((d >= 16) & (d == np.floor(d)))
            far = far[np.argsort(-d[far], kind="stable")][:24]
            if not (len(one) and len(odd)) or int(d[far].sum()) * TOP < rest:
                continue
            scan = np.zeros((NCLS, P), np.float32)
            left = rest
            for b in far:                                # whole distances: V = d 2^23
                c = min(TOP, left // int(d[b]))
                scan[cls, b] = c
                left -= c * int(d[b])
            assert left < TOP
            scan[cls, one[0]] = left
            scan[cls, odd[0]] = c_odd
            return scan, cls, T
        raise AssertionError("particle 0's window holds no class with cells at 1, at sqrt 2 and enough far ones")

    # a last-bit change of one class sum does not always reach the weight's last bit: the first H whose weight shows it
    for _ in range(200):
        scan, cls, T = build(int(rng.integers(2 ** 22, 2 ** 23)) * 2)
        one = dict(case, scan=scan, states=case["states"][:1])
        if exact_weights(oracle, one)[0] != exact_weights(oracle, one, through_double=True)[0]:
            break
    else:
        raise AssertionError("no made total whose weight depends on rounding once")
    case["made_total"] = (cls, T)
    return scan


# ---- maps -----------------------------------------------------------------------------------------------------------------
def _dict_map(rng, size, top):
    """Hand-made maps of few dyadic values in 8 x 8-cell tiles; class 0 mostly the largest; an unknown rectangle."""
    vals = np.asarray(DICT_VALUES + (top,), np.float32)
    t = size // 8
    maps = np.empty((NCLS, size, size), np.float32)
    for c in range(NCLS):
        pick = rng.integers(0, len(vals), (t, t))
        if c == 0:
            pick = np.where(rng.random((t, t)) < 0.9, len(vals) - 1, pick)
        maps[c] = np.kron(vals[pick], np.ones((8, 8), np.float32))
    mask = np.zeros((size, size), np.uint8)
    mask[20:50, 100:140] = 1
    maps[:, mask == 1] = 0
    return maps, mask


def window_of(oracle, case, st):
    """(dists, mask, src): the particle's window and the window cell each scan bin pairs with."""
    cx, cy, scale = int_exact_ref._centre(st)
    om = oracle.OracleMap(case["maps"], case["mask"], 1.0)
    if case["kind"] == "polar":
        nb, nr = case["shape"]
        dists, mask = oracle.local_map_polar(om, case["tab"], cx, cy, scale, case["res"])
        s = oracle.rot_shift(float(st["theta"]), nb)
        k = np.arange(nb * nr)
        return dists, mask, (k % nb - s) % nb + nb * (k // nb)
    rows, cols = case["shape"]
    dists, mask = oracle.local_map_cart(om, cx, cy, float(st["theta"]), np.float32(case["res"]) * scale, rows, cols)
    return dists, mask, np.arange(rows * cols)


_CACHE = {}


def make_case(oracle, name, kind):
    """dict: name, kind, form, shape, P, res, ang_res, tab (polar), maps, mask, scan, states, params (FilterParams keywords)."""
    if (name, kind) in _CACHE:
        return _CACHE[name, kind]
    form, scan_name, map_name, shape_p, shape_c = TABLE[name]
    polar = kind == "polar"
    a, b = shape_p if polar else shape_c
    wrap = scan_name == "wrap"
    size = 260 if wrap else (160 if map_name != "scene" else 200)
    seed = 7100 + 13 * NAMES.index(name) + (0 if polar else 5)
    res = (0.4 if wrap else 1.0) if polar else 0.75
    cfg = synth.Config(name, 100, NCLS, a, b, size, N_PARTICLES, polar=polar, seed=seed, res=res)
    sc = synth.make_scene(cfg)
    rng = np.random.default_rng(seed)
    maps, mask = sc.class_maps, sc.class_mask
    if map_name != "scene":
        maps, mask = _dict_map(rng, size, DICT_TOP if map_name == "dict_edge" else np.float32(512.0))
    n = N_PARTICLES
    st = synth.make_particles(cfg, sc.lab, sc.pose, rng, n=n, sigma_px=8.0 if not polar else 30.0, uniform_frac=0.1)
    far = rng.random(n) < 0.1                              # partly outside the map: clamped samples
    far[0] = False
    st["init_x_px"][far] = rng.uniform(-0.3 * size, 1.3 * size, int(far.sum())).astype(np.float32)
    wild = rng.random(n) < 0.05                            # many turns, negative headings
    wild[0] = False
    st["theta"][wild] = rng.uniform(-40, 40, int(wild.sum())).astype(np.float32)
    st["init_x_px"][1:5] = np.asarray([-0.25 * size, 2.5, size - 0.5, 0.5 * size], np.float32)    # off / at the border
    st["init_y_px"][1:5] = np.asarray([0.5 * size, 0.5 * size, 0.5 * size, -0.2 * size], np.float32)
    if not polar:
        st["scale"] = rng.uniform(0.9, 1.1, n).astype(np.float32)
    st["init_x_px"][0], st["init_y_px"][0], st["theta"][0], st["scale"][0] = sc.pose[0], sc.pose[1], sc.pose[2], 1.0
    case = dict(name=name, kind=kind, form=form, shape=(a, b), P=a * b, res=float(res), ang_res=cfg.ang_res, maps=maps,
                mask=mask, states=st, params=dict(fixed_scale=1.0),
                tab=oracle.polar_table(a, b, cfg.ang_res) if polar else None)
    case["scan"] = _past_2p53(oracle, case, rng) if scan_name == "past_2p53" else make_scan(scan_name, rng, a * b)
    _CACHE[name, kind] = case
    return case


def oracle_weights(oracle, case):
    fp = oracle.make_params(NCLS, **case["params"])
    om = oracle.OracleMap(case["maps"], case["mask"], 1.0)
    with np.errstate(all="ignore"):
        if case["kind"] == "polar":
            nb, nr = case["shape"]
            return oracle.compute_weights(om, case["tab"], nb, nr, case["scan"], case["res"], fp, case["states"].copy())
        rows, cols = case["shape"]
        return oracle.compute_weights_cart(om, rows, cols, case["scan"], case["res"], fp, case["states"].copy())


def exact_weights(oracle, case, **kw):
    fp = oracle.make_params(NCLS, **case["params"])
    if case["kind"] == "polar":
        nb, nr = case["shape"]
        return int_exact_ref.weights_polar(oracle, case["maps"], case["mask"], 1.0, case["tab"], nb, nr, case["scan"],
                                           case["res"], fp, case["states"], **kw)
    rows, cols = case["shape"]
    return int_exact_ref.weights_cart(oracle, case["maps"], case["mask"], 1.0, rows, cols, case["scan"], case["res"], fp,
                                      case["states"], **kw)


_REF = {}


def references(oracle, name, kind):
    """(case, exact reference weights, oracle weights): computed once, shared, never written to."""
    if (name, kind) not in _REF:
        case = make_case(oracle, name, kind)
        exact, orc = exact_weights(oracle, case), oracle_weights(oracle, case)
        exact.setflags(write=False)
        orc.setflags(write=False)
        _REF[name, kind] = (case, exact, orc)
    return _REF[name, kind]
