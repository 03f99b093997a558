"""Map fusion over the handle layer (include/tdr.h, "map fusion"): localised scans vote into per-class count planes over
the map's cells, and apply() relabels the cells with a verdict through the incremental map update.

    m = MapHandle.from_labels(label_img, flatten_lut, ncls); m.sample_pts_polar(nb, nr, ang_res)
    fuser = MapFuser(m, class_label, min_votes=3, share=(1, 2))
    fuser.add_scan(renderer, (cx, cy, theta, scale), res)        # or add_scans(renderers, poses) for K robots
    changed = fuser.apply(filters)                               # the filters score against the new map from now on
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

_vp = C.c_void_p


def _ptr(a):
    return a.ctypes.data_as(_vp)


class MapFuser:
    """tdr_fuser on a MapHandle last set from a label image.  class_label[c]: the raw label written for class c (the
    inverse of the map's flatten_lut); a cell is relabelled when it holds at least min_votes votes and its most-voted
    class has at least share[0] / share[1] of them."""

    def __init__(self, map_handle, class_label, min_votes=1, share=(1, 2)):
        self.L = _lib.load()
        self.map = map_handle
        self.h = _vp()
        cl = np.ascontiguousarray(class_label, np.uint8)
        if cl.size < map_handle.ncls:
            raise ValueError(f"MapFuser: class_label needs {map_handle.ncls} entries (has {cl.size})")
        check(self.L.tdr_fuser_create(map_handle.h, _ptr(cl), int(min_votes), int(share[0]), int(share[1]), C.byref(self.h)))

    def add_scan(self, renderer, pose, res):
        """The renderer's last render at pose = (cx, cy, theta, scale): (votes added, votes dropped)."""
        a, d = C.c_uint64(), C.c_uint64()
        cx, cy, th, sc = (float(x) for x in pose)
        check(self.L.tdr_fuser_add(self.h, renderer.h, C.c_float(cx), C.c_float(cy), C.c_float(th), C.c_float(sc),
                                   C.c_float(res), C.byref(a), C.byref(d)))
        return a.value, d.value

    def add_scan_from_filter(self, renderer, filter_handle, res):
        """... at the filter's max-likelihood state {x, y, theta, scale} (tdr_filter_mean_cov about the maximum)."""
        best, _ = filter_handle.mean_cov(about_max=True)
        return self.add_scan(renderer, best, res)

    def add_scans(self, renderers, poses):
        """K renders in one launch; poses[k] = (cx, cy, theta, scale, res)."""
        arr = (_vp * len(renderers))(*[r.h for r in renderers])
        p = np.ascontiguousarray(poses, np.float32).reshape(len(renderers), 5)
        a, d = C.c_uint64(), C.c_uint64()
        check(self.L.tdr_fuser_add_batch(self.h, arr, len(renderers), _ptr(p), C.byref(a), C.byref(d)))
        return a.value, d.value

    def add_images(self, imgs, polar, pose, res):
        """Host images (ncls, rows, cols) as renderSemanticTopDown fills them."""
        imgs = np.asarray(imgs, np.float32)
        ncls, rows, cols = imgs.shape
        if ncls != self.map.ncls:
            raise _lib.TdrError(f"add_images: {ncls} classes on a map of {self.map.ncls}")
        cm = np.ascontiguousarray(np.transpose(imgs, (0, 2, 1)))
        a, d = C.c_uint64(), C.c_uint64()
        cx, cy, th, sc = (float(x) for x in pose)
        check(self.L.tdr_fuser_add_images(self.h, _ptr(cm), int(bool(polar)), rows, cols, C.c_float(cx), C.c_float(cy),
                                          C.c_float(th), C.c_float(sc), C.c_float(res), C.byref(a), C.byref(d)))
        return a.value, d.value

    def apply(self, filters=()):
        """The label pass over the dirty tiles, the changed rectangle into the map and the listed filters: changed cells."""
        ch = C.c_int64(0)
        arr = (_vp * max(1, len(filters)))(*[f.h for f in filters])
        check(self.L.tdr_fuser_apply(self.h, arr if filters else None, len(filters), C.byref(ch)))
        return ch.value

    def decay(self, shift):
        check(self.L.tdr_fuser_decay(self.h, int(shift)))

    def reset(self):
        check(self.L.tdr_fuser_reset(self.h))

    def rebase(self):
        """The map's present label image becomes the base; True when the votes were kept."""
        kept = C.c_int(0)
        check(self.L.tdr_fuser_rebase(self.h, C.byref(kept)))
        return bool(kept.value)

    def stats(self):
        out = np.zeros(9, np.uint64)
        check(self.L.tdr_fuser_stats(self.h, _ptr(out)))
        names = ("scans", "votes_added", "votes_dropped", "applies", "ncls", "rows", "cols", "img_h", "img_w")
        return dict(zip(names, (int(x) for x in out)))

    def votes(self):
        """(ncls, rows, cols) uint32: cell (yi, xi) of class c at [c, yi, xi]."""
        s = self.stats()
        out = np.zeros((s["ncls"], s["rows"], s["cols"]), np.uint32)
        check(self.L.tdr_fuser_get_votes(self.h, _ptr(out)))
        return out

    def labels(self):
        """The fused label image as of the last apply, (img_h, img_w) uint8."""
        s = self.stats()
        out = np.zeros((s["img_h"], s["img_w"]), np.uint8)
        check(self.L.tdr_fuser_get_labels(self.h, _ptr(out)))
        return out

    def __del__(self):
        if getattr(self, "h", None):
            self.L.tdr_fuser_destroy(self.h)
            self.h = None
