"""What map fusion must give (include/tdr.h, "map fusion"), restated in NumPy; shared by tests/test_fuse_ref.py (which holds
this file to account) and tests/test_fuse.py (the device against it, byte for byte); not a test module.

Polar addressing is oracle/np_oracle.py's (polar_table, rot_shift, round_half_away, the expressions of local_map_polar);
the Cartesian window's sample points are the CPU oracle's sample_pts, addressed the way its local_map_cart does."""
import numpy as np

from oracle import np_oracle as no

f32 = np.float32
TILE = 32


def counts(scan):
    """n = (uint32)v when 1 <= v < 2^31, otherwise 0 (NaN, negatives, fractions below 1)."""
    v = np.asarray(scan, f32)
    with np.errstate(invalid="ignore"):
        ok = (v >= 1) & (v < 2.0 ** 31)
    return np.where(ok, np.trunc(np.where(ok, v, 0)), 0).astype(np.uint64)


def _cells(p0, p1, rows, cols):
    ri = no.round_half_away(p0).astype(np.int64)
    ci = no.round_half_away(p1).astype(np.int64)
    return ri, ci, (ri >= 0) & (ri < rows) & (ci >= 0) & (ci < cols)


def polar_cells(tab, nb, nr, resolution, rows, cols, cx, cy, theta, scale, res):
    """Per scan bin b = i + nb * j: the cell (ri, ci) of window sample ((i - s) mod nb) + nb * j and whether it is on the
    map.  tab: np_oracle.polar_table(nb, nr, ang_res, resolution)."""
    s = no.rot_shift(theta, nb)
    b = np.arange(nb * nr)
    k = (b % nb - s) % nb + nb * (b // nb)
    p0 = ((tab[0][k] * f32(scale)).astype(f32) * f32(res)).astype(f32)
    p1 = ((tab[1][k] * f32(scale)).astype(f32) * f32(res)).astype(f32)
    p0 = (p0 + f32(cy) / f32(resolution)).astype(f32)
    p1 = (p1 + f32(cx) / f32(resolution)).astype(f32)
    return _cells(p0, p1, rows, cols)


def cart_cells(oracle, win_rows, win_cols, resolution, rows, cols, cx, cy, theta, scale, res):
    """Per sample k = i + win_rows * j of the Cartesian window at rot = theta and res * scale."""
    r = f32(f32(res) * f32(scale))
    pts = oracle.sample_pts(f32(cx) / f32(resolution), f32(cy) / f32(resolution), f32(theta), win_cols, win_rows,
                            r / f32(resolution))
    return _cells(pts[:, 0], pts[:, 1], rows, cols)


def add_votes(votes, scan, cells):
    """votes (ncls, rows, cols) uint32, in place, wrapping at 2^32; scan (ncls, P).  Returns (added, dropped)."""
    ri, ci, inb = cells
    n = counts(scan)
    acc = votes.astype(np.uint64)
    for c in range(n.shape[0]):
        np.add.at(acc[c], (ri[inb], ci[inb]), n[c][inb])
    votes[...] = (acc & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return int(n[:, inb].sum()), int(n[:, ~inb].sum())


def dirty_tiles(scan, cells, cols):
    """the tiles a scan marks: those of the on-map cells that receive a non-zero count"""
    ri, ci, inb = cells
    hit = inb & (counts(scan).sum(0) > 0)
    tx_n = (cols + TILE - 1) // TILE
    return sorted(set(((ri[hit] // TILE) * tx_n + ci[hit] // TILE).tolist()))


def cell_pixels(img_h, img_w, resolution):
    """(iy, ix): the image pixel row of map row yi, the pixel column of map column xi (top_down_map.cpp:137-138)."""
    res = f32(resolution)
    rows, cols = int(f32(img_h) / res), int(f32(img_w) / res)
    iy = np.maximum((f32(img_h) - np.arange(rows).astype(f32) * res - f32(1)).astype(f32).astype(np.int64), 0)
    ix = np.minimum((np.arange(cols).astype(f32) * res).astype(f32).astype(np.int64), img_w - 1)
    return iy, ix


def verdicts(votes, min_votes, share_num, share_den):
    """(winner (rows, cols), verdict (rows, cols) bool): most votes, the lowest class on a tie; total >= min_votes and
    v_w * den >= total * num in exact integers."""
    v = votes.astype(np.uint64)
    total = v.sum(0)
    w = np.argmax(v, 0)                                  # the first maximum
    vw = np.take_along_axis(v, w[None], 0)[0]
    exact = np.vectorize(lambda a, t: int(a) * int(share_den) >= int(t) * int(share_num), otypes=[bool])
    return w, (total >= np.uint64(min_votes)) & exact(vw, total)


def fuse_labels(votes, base_img, class_label, min_votes, share_num, share_den, resolution):
    """The fused label image: a function of (votes, base) alone."""
    base_img = np.asarray(base_img, np.uint8)
    iy, ix = cell_pixels(base_img.shape[0], base_img.shape[1], resolution)
    w, ok = verdicts(votes, min_votes, share_num, share_den)
    out = base_img.copy()
    cur = out[iy[:, None], ix[None, :]]
    out[iy[:, None], ix[None, :]] = np.where(ok, np.asarray(class_label, np.uint8)[w], cur)
    return out


def class_words(img, lut, ncls, resolution):
    iy, ix = cell_pixels(img.shape[0], img.shape[1], resolution)
    c = np.asarray(lut, np.int64)[img[iy[:, None], ix[None, :]].astype(np.int64)]
    return np.where((c >= 0) & (c < ncls), c, -1)


def changed_cells(a, b, lut, ncls, resolution):
    """what tdr_map_patch_labels reports between two label images: the cells whose class changed"""
    return int((class_words(a, lut, ncls, resolution) != class_words(b, lut, ncls, resolution)).sum())


# ---- the closed loop: a stale map, scans of the truth at known poses ---------------------------------------------------------
LOOP = dict(size=160, ncls=4, nb=64, nr=24, res=1.0, seed=77, n_pts=6000, block=(70, 84, 66, 82), wrong=0, right=2,
            min_votes=2, share=(1, 2))


def closed_loop_scene():
    """A 160 x 160 synth map (resolution 1) whose TRUE labels hold a building block (class `right`, map rows 70-83, columns
    66-81) that the stale BASE image shows as terrain (class `wrong`); four true poses around the block; the polar scan
    (np_oracle.raster_polar of a synth scan of the true map) seen from each."""
    from top_down_renderer_amd import synth

    p = LOOP
    rng = np.random.default_rng(p["seed"])
    lab = synth.make_label_image(p["size"], p["ncls"], rng)
    y0, y1, x0, x1 = p["block"]
    true = lab.copy()
    true[y0 - 20:y1 + 20, x0 - 20:x1 + 20] = np.where(true[y0 - 20:y1 + 20, x0 - 20:x1 + 20] == p["right"], p["wrong"],
                                                      true[y0 - 20:y1 + 20, x0 - 20:x1 + 20])   # the block stands alone
    stale = true.copy()
    true[y0:y1, x0:x1] = p["right"]
    stale[y0:y1, x0:x1] = p["wrong"]
    unknown_id = 200

    def img(a):   # the cv::Mat layout: row 0 = top
        return np.where(a >= 0, a, unknown_id).astype(np.uint8)[::-1].copy()

    cfg = synth.Config("fuse_loop", p["n_pts"], p["ncls"], p["nb"], p["nr"], p["size"], 1, seed=p["seed"], res=p["res"])
    lut = synth.make_lut(p["ncls"])
    cyc, cxc = 0.5 * (y0 + y1), 0.5 * (x0 + x1)
    poses = [(cxc - 17.25, cyc + 1.5, 0.3), (cxc + 16.5, cyc - 2.25, -2.1), (cxc + 0.75, cyc + 15.5, 1.7),
             (cxc - 1.5, cyc - 15.25, 4.0)]
    pts = [synth.make_scan(cfg, true, ps, rng) for ps in poses]
    scans = [no.raster_polar(q, cfg.res, cfg.ang_res, lut, p["ncls"], p["nb"], p["nr"]) for q in pts]
    return dict(p, base_img=img(stale), true_img=img(true), lut=lut, ang_res=cfg.ang_res, poses=poses, pts=pts, scans=scans,
                class_label=np.arange(p["ncls"], dtype=np.uint8))


def closed_loop_fuse(sc, scans=None):
    """votes of the four scans (or of `scans` in their place) and the fused image, in NumPy"""
    rows = cols = sc["size"]
    tab = no.polar_table(sc["nb"], sc["nr"], sc["ang_res"], 1.0)
    votes = np.zeros((sc["ncls"], rows, cols), np.uint32)
    for (cx, cy, th), scan in zip(sc["poses"], sc["scans"] if scans is None else scans):
        add_votes(votes, scan, polar_cells(tab, sc["nb"], sc["nr"], 1.0, rows, cols, cx, cy, th, 1.0, sc["res"]))
    fused = fuse_labels(votes, sc["base_img"], sc["class_label"], sc["min_votes"], sc["share"][0], sc["share"][1], 1.0)
    return votes, fused


def pose_cost(class_maps, class_mask, sc, k):
    """the oracle's getCostForRot of scan k at its true pose on a map"""
    cx, cy, th = sc["poses"][k]
    tab = no.polar_table(sc["nb"], sc["nr"], sc["ang_res"], 1.0)
    d, m = no.local_map_polar(class_maps, class_mask, 1.0, tab, cx, cy, 1.0, sc["res"])
    maskf = (f32(1) - m.astype(f32)).astype(f32)
    return float(no.cost_for_rot(sc["scans"][k], d, maskf, sc["nb"], sc["nr"], np.ones(sc["ncls"], f32), th))
