"""NumPy restatement of sensor resetting (include/tdr.h, "sensor resetting"): the list of injected slots, the candidates of
a slot, the pick among their weights, the write.  Written from the definition, not from the kernels; the weights of the
candidates are an INPUT here (whoever calls decides which scorer gives them).  Philox and the road list come from the
restatement of the recovery injection.  Not a test module."""
import numpy as np

import recovery_ref as RR

F32 = RR.F32
U64 = RR.U64
FIELDS = ("init_x_px", "init_y_px", "dx_m", "dy_m", "theta", "scale", "have_init")


def _words(seed, draw):
    return (seed & 0xFFFFFFFF, seed >> 32), (draw & 0xFFFFFFFF, draw >> 32)


def inject_list(n, slot_begin, seed, draw, threshold24):
    """Rule 1: the LOCAL indices of the injected slots of [0, n), ascending (int64)."""
    if n == 0 or threshold24 == 0:
        return np.zeros(0, np.int64)
    key, d = _words(seed, draw)
    i = (np.arange(n, dtype=U64) + U64(slot_begin)) & RR.M32
    a0 = RR.philox((i, d[0], d[1], 0), key)[0]
    return np.flatnonzero((a0 >> np.uint32(8)).astype(np.int64) < int(threshold24)).astype(np.int64)


def candidates(states, lst, C, slot_begin, road, cols, resolution, seed, draw, heading_mode):
    """Rules 2 and 3: the candidates of the listed slots as a STATE_DTYPE array of shape (len(lst), C)."""
    lst = np.asarray(lst, np.int64)
    road = np.asarray(road, np.uint32)
    key, d = _words(seed, draw)
    i = ((lst.astype(U64) + U64(slot_begin)) & RR.M32)[:, None]
    j = np.arange(C, dtype=U64)[None, :]
    a = RR.philox((i, d[0], d[1], U64(2) * j), key)
    cell = road[((a[1].astype(U64) * U64(len(road))) >> U64(32)).astype(np.int64)]
    r, c = cell // np.uint32(cols), cell % np.uint32(cols)
    ux = (a[2] >> np.uint32(24)).astype(F32) * F32(2.0 ** -8)
    uy = (a[3] >> np.uint32(24)).astype(F32) * F32(2.0 ** -8)
    out = np.zeros((len(lst), C), RR.STATE_DTYPE)
    out["init_x_px"] = (c.astype(F32) + ux) * F32(resolution)
    out["init_y_px"] = (r.astype(F32) + uy) * F32(resolution)
    out["scale"] = states["scale"][lst][:, None]
    if heading_mode == 1:
        b = RR.philox((i, d[0], d[1], U64(2) * j + U64(1)), key)
        out["theta"] = (b[0] >> np.uint32(8)).astype(F32) * F32(2.0 ** -24) * F32(6.2831855) - F32(3.1415927)
        out["have_init"] = 1
    return out


def pick(weights):
    """Rule 5 on rows of weights (m, C): per row the smallest j whose key (the weight; -1 for a NaN) is the maximum."""
    w = np.asarray(weights, F32)
    key = np.where(np.isnan(w), F32(-1), w)
    return np.argmax(key, axis=1)          # the first of equal maxima


def write(states, lst, cand_after, picks):
    """Rule 6: the listed slots take the picked candidates' fields as scoring left them (cand_after: (m, C))."""
    out = states.copy()
    lst = np.asarray(lst, np.int64)
    win = cand_after[np.arange(len(lst)), np.asarray(picks, np.int64)]
    for name in FIELDS:
        out[name][lst] = win[name]
    return out


def inject_sensor(states, n, slot_begin, road, cols, resolution, seed, draw, threshold24, heading_mode, C, score):
    """The whole rule on slots [0, n).  score(cand_flat) -> (weights, cand_flat as scoring left them) for a flat STATE_DTYPE
    array of candidates.  Returns (the new array, the list, the picks)."""
    lst = inject_list(n, slot_begin, seed, draw, threshold24)
    if len(lst) == 0:
        return states.copy(), lst, np.zeros(0, np.int64)
    cand = candidates(states, lst, C, slot_begin, road, cols, resolution, seed, draw, heading_mode)
    w, after = score(cand.reshape(-1))
    picks = pick(np.asarray(w, F32).reshape(len(lst), C))
    return write(states, lst, np.asarray(after).reshape(len(lst), C), picks), lst, picks
