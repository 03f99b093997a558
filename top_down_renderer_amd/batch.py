"""Batched filters over the handle layer (include/tdr.h: tdr_batch_step): many filters that share one map stepped
together — propagate + update of every filter, one launch per stage for those that qualify, the standalone calls for the
others.  Each filter ends bit for bit where tdr_filter_propagate + tdr_filter_update would leave it.

    m = MapHandle(class_maps, class_mask, resolution=1.0); m.sample_pts_polar(100, 25, ang_res)
    fs = [FilterHandle(m, 20000, params, seed=s) for s in seeds]   # set_states / initialize_particles
    step_batch(fs, scans, res, priors)                              # scans[k]: (ncls, nb, nr) array, or a Renderer

The node loop of many robots (tdr_batch_render_polar + tdr_batch_step + tdr_batch_pose):

    loop = LoopBatch(filters, renderers, cfgs, ang_res, ncls, nb, nr)
    ests = loop.take_step(clouds, priors)       # one PoseEst per robot, as TopDownRenderCore.takeStep returns it
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import BatchCloudC, BatchInputC, FilterParamsC, PoseStatsC, VizRequestC, check
from .particle_filter import GridResult, kld_params_c, recovery_params_c

_vp = C.c_void_p
STATE_DTYPE = np.dtype([("init_x_px", "<f4"), ("init_y_px", "<f4"), ("dx_m", "<f4"), ("dy_m", "<f4"), ("theta", "<f4"),
                        ("scale", "<f4"), ("have_init", "u1"), ("pad", "u1", 3)])


def _ptr(a):
    return a.ctypes.data_as(_vp)


class MapHandle:
    """tdr_map: class_maps (ncls, rows, cols) distance maps, class_mask (rows, cols) with 1 = unknown."""

    def __init__(self, class_maps, class_mask, resolution=1.0, center=(0, 0)):
        self.L = _lib.load()
        self.h = _vp()
        check(self.L.tdr_map_create(C.byref(self.h)))
        ncls, rows, cols = class_maps.shape
        maps_cm, mask_cm = _maps_cm(class_maps, class_mask)
        check(self.L.tdr_map_set(self.h, _ptr(maps_cm), _ptr(mask_cm), ncls, rows, cols, C.c_float(resolution),
                                 int(center[0]), int(center[1])))
        self.ncls = ncls

    @classmethod
    def from_labels(cls, label_img, flatten_lut, ncls, resolution=1.0, center=(0, 0)):
        """A map set from a class-index image (tdr_map_set_labels; cv::Mat layout, row 0 = top)."""
        self = cls.__new__(cls)
        self.L = _lib.load()
        self.h = _vp()
        check(self.L.tdr_map_create(C.byref(self.h)))
        img, lut = _label_args(label_img, flatten_lut)
        check(self.L.tdr_map_set_labels(self.h, _ptr(img), img.shape[0], img.shape[1], _ptr(lut), len(lut), int(ncls),
                                        C.c_float(resolution), int(center[0]), int(center[1])))
        self.ncls = int(ncls)
        return self

    def center(self):
        """mapCenter() (tdr_map_center): (center_x, center_y)."""
        cx, cy = C.c_int(), C.c_int()
        check(self.L.tdr_map_center(self.h, C.byref(cx), C.byref(cy)))
        return cx.value, cy.value

    def road_cells(self):
        """The map's road list (tdr_map_road_cells) read back: ascending cell indices r * cols + c, uint32."""
        n = C.c_int64(0)
        check(self.L.tdr_map_read_road_cells(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint32)
        check(self.L.tdr_map_read_road_cells(self.h, _ptr(out), n.value, C.byref(n)))
        return out

    def sample_pts_polar(self, nb, nr, ang_res):
        check(self.L.tdr_map_sample_pts_polar(self.h, nb, nr, C.c_float(ang_res)))
        self.shape = (nb, nr)

    def set_window(self, rows, cols):
        """The Cartesian window (tdr_map_set_window) a FilterHandle(..., cart=True) scores against."""
        check(self.L.tdr_map_set_window(self.h, int(rows), int(cols)))
        self.window = (int(rows), int(cols))

    def set_viz_background(self, bgr=None, labels=None, lut=None):
        """The fleet picture's background, one device copy for every filter on this map: bgr (H, W, 3) uint8, or labels
        (H, W) uint8 coloured on the device through lut (256 BGR triplets).  It stays until it is set again."""
        if labels is not None:
            labels = np.ascontiguousarray(labels, np.uint8)
            lut = np.ascontiguousarray(lut, np.uint8).ravel()
            if labels.ndim != 2 or lut.size != 768:
                raise ValueError("set_viz_background: labels (H, W) and 256 BGR triplets")
            check(self.L.tdr_map_set_viz_background_labels(self.h, _ptr(labels), labels.shape[0], labels.shape[1], _ptr(lut)))
            return
        bgr = np.ascontiguousarray(bgr, np.uint8)
        if bgr.ndim != 3 or bgr.shape[2] != 3:
            raise ValueError("set_viz_background: a (H, W, 3) BGR image")
        check(self.L.tdr_map_set_viz_background(self.h, _ptr(bgr), bgr.shape[0], bgr.shape[1]))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.tdr_map_destroy(self.h)
            self.h = None


def _maps_cm(class_maps, class_mask):
    """(ncls, rows, cols) distance maps and the (rows, cols) mask in the column-major layout tdr_map_set reads."""
    return (np.ascontiguousarray(np.transpose(class_maps, (0, 2, 1)), np.float32),
            np.ascontiguousarray(np.asarray(class_mask).T, np.uint8))


def _label_args(label_img, flatten_lut):
    img = np.ascontiguousarray(label_img, np.uint8)
    if img.ndim != 2:
        raise ValueError("a label image is (H, W) uint8")
    return img, np.ascontiguousarray(flatten_lut, np.int32).ravel()


class Renderer:
    """tdr_renderer whose last render stays on the device (a batch input that needs no host images)."""

    def __init__(self, lut256):
        self.L = _lib.load()
        self.h = _vp()
        self._lut = np.ascontiguousarray(lut256, np.int32)
        check(self.L.tdr_renderer_create(_ptr(self._lut), C.byref(self.h)))
        self._shape = None

    def render_polar(self, pts, stride, ioff, res, ang_res, ncls, nb, nr):
        """pts: points of `stride` floats, x y z at 0..2, the label at float `ioff`."""
        pts = np.ascontiguousarray(pts, np.float32)
        self._shape = (ncls, nb, nr)
        check(self.L.tdr_renderer_render(self.h, 1, _ptr(pts), stride, ioff, pts.size // stride, C.c_float(res),
                                         C.c_float(ang_res), ncls, nb, nr, None))

    def render_cart(self, pts, stride, ioff, res, ncls, rows, cols):
        """ScanRenderer::renderSemanticTopDown: the Cartesian render a Cartesian filter reads."""
        pts = np.ascontiguousarray(pts, np.float32)
        self._shape = (ncls, rows, cols)
        check(self.L.tdr_renderer_render(self.h, 0, _ptr(pts), stride, ioff, pts.size // stride, C.c_float(res),
                                         C.c_float(1.0), ncls, rows, cols, None))

    def get_render(self):
        """(img, pk) of the last render: img (ncls, rows, cols) as renderSemanticTopDown fills it, pk (rows * cols, rf) the
        packed records the scoring reads (record t = row + rows * col)."""
        shape = self._shape
        if shape is None:
            raise _lib.TdrError("get_render: the renderer has no render")
        ncls, nb, nr = shape
        img = np.zeros((ncls, nr, nb), np.float32)
        pk = np.zeros((nb * nr, self.L.tdr_rec_floats(ncls)), np.float32)
        check(self.L.tdr_renderer_get_render(self.h, _ptr(img), _ptr(pk)))
        return np.ascontiguousarray(np.transpose(img, (0, 2, 1))), pk

    def picture(self, unflatten, lut_bgr):
        """The scan picture of the last render (tdr_renderer_visualize): a (cols, rows, 3) uint8 BGR array."""
        unf, lut = _picture_tables(unflatten, lut_bgr, self._shape[0] if self._shape else 0)
        oh, ow = C.c_int(), C.c_int()
        check(self.L.tdr_renderer_visualize(self.h, _ptr(unf), _ptr(lut), None, 0, C.byref(oh), C.byref(ow)))
        out = np.zeros((oh.value, ow.value, 3), np.uint8)
        check(self.L.tdr_renderer_visualize(self.h, _ptr(unf), _ptr(lut), _ptr(out), out.size, C.byref(oh), C.byref(ow)))
        return out

    def picture_analog(self, cls, scale):
        """visualizeAnalog of class layer `cls` of the last render (tdr_renderer_visualize_analog)."""
        oh, ow = C.c_int(), C.c_int()
        check(self.L.tdr_renderer_visualize_analog(self.h, int(cls), C.c_float(scale), None, 0, C.byref(oh), C.byref(ow)))
        out = np.zeros((oh.value, ow.value, 3), np.uint8)
        check(self.L.tdr_renderer_visualize_analog(self.h, int(cls), C.c_float(scale), _ptr(out), out.size, C.byref(oh),
                                                   C.byref(ow)))
        return out

    def __del__(self):
        if getattr(self, "h", None):
            self.L.tdr_renderer_destroy(self.h)
            self.h = None


def _picture_tables(unflatten, lut_bgr, ncls):
    unf = np.ascontiguousarray(unflatten, np.int32).ravel()
    lut = np.ascontiguousarray(lut_bgr, np.uint8).ravel()
    if unf.size < ncls or lut.size != 768:
        raise ValueError(f"pictures: unflatten needs {ncls} entries (has {unf.size}), the colour table 256 BGR triplets")
    return unf, lut


class FilterHandle:
    """tdr_filter on a MapHandle; seed != 0 is the reference-ordered generator (parity mode).  cart: the Cartesian filter
    (tdr_filter_create_cart) over the map's window (MapHandle.set_window)."""

    def __init__(self, map_handle, n_max, params, seed=0, cart=False):
        self.L = _lib.load()
        self.map = map_handle
        self.cart = bool(cart)
        self.h = _vp()
        fp = params if isinstance(params, FilterParamsC) else params.to_c(map_handle.ncls)
        create = self.L.tdr_filter_create_cart if cart else self.L.tdr_filter_create
        check(create(map_handle.h, int(n_max), C.byref(fp), int(seed), C.byref(self.h)))

    def initialize_particles(self):
        check(self.L.tdr_filter_initialize_particles(self.h))

    def configure(self, parity_rng, locality_every=1):
        check(self.L.tdr_filter_configure(self.h, int(parity_rng), int(locality_every)))

    def set_states(self, states):
        states = np.ascontiguousarray(states, STATE_DTYPE)
        check(self.L.tdr_filter_set_states(self.h, _ptr(states), len(states)))

    def num_particles(self):
        return int(self.L.tdr_filter_num_particles(self.h))

    def states(self):
        out = np.zeros(self.num_particles(), STATE_DTYPE)
        check(self.L.tdr_filter_get_states(self.h, _ptr(out), len(out)))
        return out

    def _floats(self, fn, n):
        out = np.zeros(n, np.float32)
        check(fn(self.h, _ptr(out), n))
        return out

    def weights(self):
        return self._floats(self.L.tdr_filter_get_weights, self.num_particles())

    def raw_weights(self, n):
        return self._floats(self.L.tdr_filter_get_raw_weights, n)

    def resample_indices(self):
        out = np.zeros(self.num_particles(), np.int32)
        check(self.L.tdr_filter_get_resample_indices(self.h, _ptr(out), len(out)))
        return out

    def mean_cov(self, about_max=False):
        st, cov = np.zeros(4, np.float32), np.zeros(16, np.float32)
        check(self.L.tdr_filter_mean_cov(self.h, int(bool(about_max)), _ptr(st), _ptr(cov)))
        return st, cov.reshape(4, 4)

    def freeze_scale(self):
        check(self.L.tdr_filter_freeze_scale(self.h))

    def is_scale_frozen(self):
        return bool(self.L.tdr_filter_is_scale_frozen(self.h))

    def scale(self):
        return float(self.L.tdr_filter_scale(self.h))

    def propagate(self, tx, ty, omega):
        check(self.L.tdr_filter_propagate(self.h, C.c_float(tx), C.c_float(ty), C.c_float(omega)))

    def propagate_freeze(self, tx, ty, omega, scale_freeze):
        """StateParticle::propagate with the caller's scale_freeze flag (tdr_filter_propagate_freeze)."""
        check(self.L.tdr_filter_propagate_freeze(self.h, C.c_float(tx), C.c_float(ty), C.c_float(omega), int(bool(scale_freeze))))

    def last_dist(self, n=None):
        """lastDist() of the first n particles (tdr_filter_get_last_dist): what the last propagate left."""
        return self._floats(self.L.tdr_filter_get_last_dist, self.num_particles() if n is None else int(n))

    def update_geo(self, scan, geo, res, n_target=-1):
        """update with the geometric images entering the score (tdr_filter_update_geo): scan (ncls, nb, nr), geo (2, nb, nr)."""
        imgs = _scan_images(scan, self.map, self.cart)
        g = np.asarray(geo, np.float32)
        if g.shape != (2,) + imgs.shape[:0:-1]:
            raise ValueError(f"geometric images of shape {g.shape}, the map expects {(2,) + imgs.shape[:0:-1]}")
        g = np.ascontiguousarray(np.transpose(g, (0, 2, 1)))
        check(self.L.tdr_filter_update_geo(self.h, _ptr(imgs), _ptr(g), C.c_float(res), int(n_target)))

    # updateMap of a live filter: the map is replaced, the particles shift by the centre's move (or are initialised)
    def update_map(self, class_maps, class_mask, resolution, center):
        """tdr_filter_update_map: the new map in distance-map form."""
        ncls, rows, cols = class_maps.shape
        maps_cm, mask_cm = _maps_cm(class_maps, class_mask)
        check(self.L.tdr_filter_update_map(self.h, _ptr(maps_cm), _ptr(mask_cm), ncls, rows, cols, C.c_float(resolution),
                                           int(center[0]), int(center[1])))
        self.map.ncls = ncls

    def update_map_labels(self, label_img, flatten_lut, ncls, resolution, center):
        """tdr_filter_update_map_labels: the new map as a class-index image (cv::Mat layout)."""
        img, lut = _label_args(label_img, flatten_lut)
        check(self.L.tdr_filter_update_map_labels(self.h, _ptr(img), img.shape[0], img.shape[1], _ptr(lut), len(lut),
                                                  int(ncls), C.c_float(resolution), int(center[0]), int(center[1])))
        self.map.ncls = int(ncls)

    def update_map_labels_incremental(self, label_img, flatten_lut, ncls, resolution, center):
        """tdr_filter_update_map_labels_incremental; returns the changed cells (-1: the full path was taken)."""
        img, lut = _label_args(label_img, flatten_lut)
        changed = C.c_int64(0)
        check(self.L.tdr_filter_update_map_labels_incremental(self.h, _ptr(img), img.shape[0], img.shape[1], _ptr(lut),
                                                              len(lut), int(ncls), C.c_float(resolution), int(center[0]),
                                                              int(center[1]), C.byref(changed)))
        self.map.ncls = int(ncls)
        return changed.value

    def patch_map_labels(self, patch, y0, x0, center):
        """tdr_filter_patch_map_labels: the rectangle at image pixel (y0, x0) of the last label image overwritten."""
        patch = np.ascontiguousarray(patch, np.uint8)
        changed = C.c_int64(0)
        check(self.L.tdr_filter_patch_map_labels(self.h, _ptr(patch), int(y0), int(x0), patch.shape[0], patch.shape[1],
                                                 int(center[0]), int(center[1]), C.byref(changed)))
        return changed.value

    def update(self, scan, res, n_target=-1):
        if isinstance(scan, Renderer):
            check(self.L.tdr_filter_update(self.h, None, scan.h, C.c_float(res), int(n_target)))
        else:
            imgs = _scan_images(scan, self.map, self.cart)
            check(self.L.tdr_filter_update(self.h, _ptr(imgs), None, C.c_float(res), int(n_target)))

    def compute_gmm(self, device=True):
        """computeGMM on the current particles: the fit on the device (tdr_filter_compute_gmm_device) or the host."""
        check((self.L.tdr_filter_compute_gmm_device if device else self.L.tdr_filter_compute_gmm)(self.h))

    def get_gmm(self):
        """(means (k, 3), covs (k, 3, 3)) of the last compute_gmm."""
        k = C.c_int()
        means, covs = np.zeros((_lib.GMM_MAX_K, 3), np.float32), np.zeros((_lib.GMM_MAX_K, 9), np.float32)
        check(self.L.tdr_filter_get_gmm(self.h, _lib.GMM_MAX_K, C.byref(k), _ptr(means), _ptr(covs)))
        return means[: k.value].copy(), covs[: k.value].reshape(-1, 3, 3).copy()

    def kld_count(self, params):
        """(k, skipped, target) of tdr_filter_kld_count: the pose bins the particles occupy, the particles without a key, the
        n_target of the next update.  params: KldParams or KldParamsC.  The filter is read, not changed."""
        p = params if isinstance(params, _lib.KldParamsC) else params.to_c()
        k, sk, t = C.c_int64(), C.c_int64(), C.c_int64()
        check(self.L.tdr_filter_kld_count(self.h, C.byref(p), C.byref(k), C.byref(sk), C.byref(t)))
        return k.value, sk.value, t.value

    def weight_stats(self):
        """The first 8 floats of the last update's info (tdr_filter_get_weight_stats): {argmax bits, sum, mean,
        bottom_stddev, fallback, num_valid, num_under, 0}."""
        out = np.zeros(8, np.float32)
        check(self.L.tdr_filter_get_weight_stats(self.h, _ptr(out)))
        return out

    def inject(self, p, heading_mode=0, seed=0, count=True):
        """tdr_filter_inject: fresh on-road particles in the slots whose Philox word falls below floor(p * 2^24).  Returns
        the number of injected slots, or None with count=False (no read-back, no wait)."""
        n = C.c_int64(0)
        check(self.L.tdr_filter_inject(self.h, C.c_double(p), int(heading_mode), int(seed), C.byref(n) if count else None))
        return n.value if count else None

    def recovery_step(self, state, params):
        """tdr_filter_recovery_step: state (a _lib.RecoveryStateC) tracks the last update's mean raw weight, and the filter
        is injected when the tracker asks for it.  params: RecoveryParams or RecoveryParamsC.  Returns (p, injected)."""
        rp = params if isinstance(params, _lib.RecoveryParamsC) else params.to_c()
        p, n = C.c_double(0), C.c_int64(0)
        check(self.L.tdr_filter_recovery_step(self.h, C.byref(state), C.byref(rp), C.byref(p), C.byref(n)))
        return p.value, n.value

    def _scan_args(self, scan):
        """(scan_imgs, renderer) of a scoring call: a Renderer, images (ncls, nb, nr), or None: the scan the filter kept."""
        if scan is None:
            return None, None, None
        if isinstance(scan, Renderer):
            return None, scan.h, None
        imgs = _scan_images(scan, self.map, self.cart)
        return _ptr(imgs), None, imgs

    def inject_sensor(self, scan, res, p, candidates, heading_mode=0, seed=0, count=True):
        """tdr_filter_inject_sensor: the slots inject() would write take the best-scoring of `candidates` road candidates
        against `scan` (a Renderer, images, or None: the scan the filter kept).  Returns the number of written slots, or
        None with count=False."""
        n = C.c_int64(0)
        imgs, rh, keep = self._scan_args(scan)
        check(self.L.tdr_filter_inject_sensor(self.h, imgs, rh, C.c_float(res), C.c_double(p), int(candidates), int(heading_mode),
                                              int(seed), C.byref(n) if count else None))
        return n.value if count else None

    def grid_search(self, scan, res, spec, nms_radius=2, max_peaks=8, vol=False):
        """tdr_filter_grid_search: `scan` (a Renderer, images, or None: the scan the filter kept) scored over the lattice of
        spec (a _lib.GridSpecC) as a particle of this filter would be, and the peaks of the weight plane.  Returns a
        particle_filter.GridResult; the filter is read, not changed."""
        nx, ny, H = int(spec.nx), int(spec.ny), int(spec.n_headings)
        G = max(nx, 0) * max(ny, 0)
        nan = np.float32("nan")
        w, t = np.full(G, nan, np.float32), np.full(G, nan, np.float32)
        v = np.full(G * max(H, 0), nan, np.float32) if vol else None
        peaks = np.zeros(max(int(max_peaks), 1), _lib.GRID_PEAK_DTYPE)
        n_peaks, listed = C.c_int64(0), C.c_int64(0)
        imgs, rh, keep = self._scan_args(scan)
        check(self.L.tdr_filter_grid_search(self.h, imgs, rh, C.c_float(res), C.byref(spec), _ptr(w), _ptr(t),
                                            _ptr(v) if vol else None, int(nms_radius), int(max_peaks), _ptr(peaks),
                                            C.byref(n_peaks), C.byref(listed)))
        return GridResult(w.reshape(ny, nx), t.reshape(ny, nx), v.reshape(H, ny, nx) if vol else None,
                          peaks[: min(int(max_peaks), n_peaks.value)].copy(), n_peaks.value, listed.value)

    def inject_cells(self, cells, p, heading_mode=0, seed=0, count=True):
        """tdr_filter_inject_cells: inject() with the caller's cell list (r * cols + c, duplicates weight the draw) in place
        of the map's road list.  Returns the number of injected slots, or None with count=False."""
        cells = np.ascontiguousarray(cells, np.uint32).ravel()
        n = C.c_int64(0)
        check(self.L.tdr_filter_inject_cells(self.h, _ptr(cells), len(cells), C.c_double(p), int(heading_mode), int(seed),
                                             C.byref(n) if count else None))
        return n.value if count else None

    def recovery_step_sensor(self, state, params, candidates, scan, res):
        """tdr_filter_recovery_step_sensor: recovery_step with inject_sensor.  Returns (p, injected)."""
        rp = params if isinstance(params, _lib.RecoveryParamsC) else params.to_c()
        p, n = C.c_double(0), C.c_int64(0)
        imgs, rh, keep = self._scan_args(scan)
        check(self.L.tdr_filter_recovery_step_sensor(self.h, C.byref(state), C.byref(rp), int(candidates), imgs, rh, C.c_float(res),
                                                     C.byref(p), C.byref(n)))
        return p.value, n.value

    def set_viz_background(self, bgr=None, labels=None, lut=None):
        """The picture's background: bgr (H, W, 3) uint8, or labels (H, W) uint8 coloured on the device through lut
        (256 BGR triplets; tdr_filter_set_viz_background_labels)."""
        if labels is not None:
            labels = np.ascontiguousarray(labels, np.uint8)
            lut = np.ascontiguousarray(lut, np.uint8).ravel()
            if labels.ndim != 2 or lut.size != 768:
                raise ValueError("set_viz_background: labels (H, W) and 256 BGR triplets")
            check(self.L.tdr_filter_set_viz_background_labels(self.h, _ptr(labels), labels.shape[0], labels.shape[1], _ptr(lut)))
            return
        bgr = np.ascontiguousarray(bgr, np.uint8)
        if bgr.ndim != 3 or bgr.shape[2] != 3:
            raise ValueError("set_viz_background: a (H, W, 3) BGR image")
        check(self.L.tdr_filter_set_viz_background(self.h, _ptr(bgr), bgr.shape[0], bgr.shape[1]))

    def visualize(self, pub_scale, arrows=None):
        """The particle picture (tdr_filter_visualize): an (out_h, out_w, 3) uint8 array."""
        arr = None if arrows is None or len(arrows) == 0 else np.ascontiguousarray(arrows, np.int32).reshape(-1, 4)
        m, ap = (0, None) if arr is None else (len(arr), _ptr(arr))
        oh, ow = C.c_int(), C.c_int()
        check(self.L.tdr_filter_visualize(self.h, C.c_float(pub_scale), ap, m, None, 0, C.byref(oh), C.byref(ow)))
        out = np.zeros((oh.value, ow.value, 3), np.uint8)
        check(self.L.tdr_filter_visualize(self.h, C.c_float(pub_scale), ap, m, _ptr(out), out.size, C.byref(oh), C.byref(ow)))
        return out

    def step_count(self):
        """The updates the filter has made (tdr_filter_step_count)."""
        return int(self.L.tdr_filter_step_count(self.h))

    def num_gaussians(self):
        return int(self.L.tdr_filter_num_gaussians(self.h))

    def set_num_gaussians(self, k):
        """num_gaussians_ (:7): the count the next compute_gmm searches around."""
        check(self.L.tdr_filter_set_num_gaussians(self.h, int(k)))

    def adaptive_count(self):
        """The particle count of :151-157 from the stored mixture (n_target of the next update)."""
        return int(self.L.tdr_filter_adaptive_count(self.h))

    def compute_weights(self, scan, res):
        """StateParticle::computeWeight for every particle (tdr_filter_compute_weights); read them with raw_weights."""
        if isinstance(scan, Renderer):
            check(self.L.tdr_filter_compute_weights(self.h, None, scan.h, C.c_float(res)))
        else:
            imgs = _scan_images(scan, self.map, self.cart)
            check(self.L.tdr_filter_compute_weights(self.h, _ptr(imgs), None, C.c_float(res)))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.tdr_filter_destroy(self.h)
            self.h = None


def _scan_images(scan, map_handle, cart=False):
    """(ncls, nb, nr) images -> the column-major [ncls][nb*nr] layout tdr_filter_update reads; the shape is checked
    (cart: against the map's window)."""
    a = np.asarray(scan, np.float32)
    want = (map_handle.ncls,) + tuple(map_handle.window if cart else map_handle.shape)
    if a.shape != want:
        raise ValueError(f"scan of shape {a.shape}, the map expects {want}")
    return np.ascontiguousarray(np.transpose(a, (0, 2, 1)))


def step_batch(filters, scans, res, priors, n_targets=None, stream=None):
    """propagate(priors[k]) + update(scans[k], res[k], n_targets[k]) of every filter in one tdr_batch_step.
    priors[k] = (tx, ty, omega); res: a float or one per filter; scans[k]: (ncls, nb, nr) images or a Renderer.
    stream: a hipStream_t as an int (None = the default stream).  Returns (batched, standalone) filter counts."""
    L = _lib.load()
    k = len(filters)
    if len(scans) != k or len(priors) != k:
        raise ValueError("step_batch: one scan and one prior per filter")
    resv = list(res) if np.ndim(res) else [float(res)] * k
    nts = [-1] * k if n_targets is None else [int(t) for t in n_targets]
    arr = (_vp * max(k, 1))(*[f.h for f in filters])
    ins = (BatchInputC * max(k, 1))()
    keep = []
    for i, (f, sc, pr) in enumerate(zip(filters, scans, priors)):
        if isinstance(sc, Renderer):
            ins[i].renderer = sc.h
        else:
            imgs = _scan_images(sc, f.map, f.cart)   # (a Cartesian filter: tdr_batch_step refuses it)
            keep.append(imgs)
            ins[i].scan_imgs = imgs.ctypes.data
        ins[i].res, ins[i].n_target = resv[i], nts[i]
        ins[i].tx, ins[i].ty, ins[i].omega = (float(v) for v in pr)
    check(L.tdr_batch_step(arr, k, ins, _vp(stream) if stream else None))
    return last_stats()


def set_init_search_in_batch(on):
    """tdr_config_tuning("batch_init_search"): with True a filter that may still hold a particle without a heading (a cold
    start, a gated filter) joins the batch, its 40-rotation search part of the batch's scoring stage — same bits; False (the
    default): it runs its standalone calls inside step_batch.  Process-wide.  Returns the value in force."""
    return bool(_lib.load().tdr_config_tuning(b"batch_init_search", 1 if on else 0))


def init_search_in_batch():
    return bool(_lib.load().tdr_config_tuning(b"batch_init_search", -1))


def last_stats():
    """(batched, standalone): how the filters of this thread's last step_batch were stepped."""
    L = _lib.load()
    a, b = C.c_int(), C.c_int()
    check(L.tdr_batch_last_stats(C.byref(a), C.byref(b)))
    return a.value, b.value


def compute_gmm_batch(filters, stream=None):
    """FilterHandle.compute_gmm(device=True) of every filter in one tdr_batch_compute_gmm: the samples, every candidate
    fit and the picks are one launch each.  The filters may be polar or Cartesian and need not share a map."""
    L = _lib.load()
    k = len(filters)
    arr = (_vp * max(k, 1))(*[f.h if f is not None else None for f in filters])
    check(L.tdr_batch_compute_gmm(arr, k, _vp(stream) if stream else None))


def kld_count(filters, params, stream=None):
    """FilterHandle.kld_count of every filter in one tdr_batch_kld_count (one job upload, one fill, one launch, one
    read-back): (k[n], skipped[n], target[n]) int64 arrays.  The filters may be polar or Cartesian and need not share a map."""
    L = _lib.load()
    n = len(filters)
    p = params if isinstance(params, _lib.KldParamsC) else params.to_c()
    arr = (_vp * max(n, 1))(*[f.h if f is not None else None for f in filters])
    k, sk, t = (np.zeros(max(n, 1), np.int64) for _ in range(3))
    check(L.tdr_batch_kld_count(arr, n, C.byref(p), _ptr(k), _ptr(sk), _ptr(t), _vp(stream) if stream else None))
    return k[:n], sk[:n], t[:n]


def inject(filters, p, heading_mode=0, seeds=None, count=True, stream=None):
    """FilterHandle.inject of every filter in one tdr_batch_inject (one job upload, one launch, one read-back): p and seeds
    one per filter (a scalar serves all).  Returns the injected counts (int64 array), or None with count=False."""
    L = _lib.load()
    n = len(filters)
    pv = np.ascontiguousarray(np.broadcast_to(np.asarray(p, np.float64), (n,)))
    sv = np.ascontiguousarray(np.broadcast_to(np.asarray(0 if seeds is None else seeds, np.uint64), (n,)))
    arr = (_vp * max(n, 1))(*[f.h if f is not None else None for f in filters])
    out = np.zeros(max(n, 1), np.int64)
    check(L.tdr_batch_inject(arr, n, _ptr(pv) if n else None, int(heading_mode), _ptr(sv) if n else None,
                             _ptr(out) if count else None, _vp(stream) if stream else None))
    return out[:n] if count else None


def render_batch(renderers, clouds, res, ang_res, ncls, nb, nr, stream=None):
    """Renderer.render_polar of every renderer in one tdr_batch_render_polar: clouds[k] = (pts, stride, ioff) with pts an
    (n, stride) float32 array (n may be 0); res: a float or one per renderer.  The renders stay on the device."""
    L = _lib.load()
    k = len(renderers)
    if len(clouds) != k:
        raise ValueError("render_batch: one cloud per renderer")
    resv = list(res) if np.ndim(res) else [float(res)] * k
    arr = (_vp * max(k, 1))(*[r.h for r in renderers])
    cs = (BatchCloudC * max(k, 1))()
    keep = []
    for i, (pts, stride, ioff) in enumerate(clouds):
        pts = np.ascontiguousarray(pts, np.float32)
        keep.append(pts)
        cs[i].pts = pts.ctypes.data if pts.size else None
        cs[i].stride, cs[i].ioff, cs[i].n, cs[i].res = int(stride), int(ioff), pts.size // int(stride), float(resv[i])
    check(L.tdr_batch_render_polar(arr, k, cs, C.c_float(ang_res), int(ncls), int(nb), int(nr),
                                   _vp(stream) if stream else None))
    for r in renderers:
        r._shape = (int(ncls), int(nb), int(nr))


def pose_batch(filters, stream=None):
    """FilterHandle.mean_cov() + scale() of every filter in one tdr_batch_pose: (mean[k, 4], cov[k, 4, 4], scale[k], n[k])."""
    L = _lib.load()
    k = len(filters)
    arr = (_vp * max(k, 1))(*[f.h for f in filters])
    out = (PoseStatsC * max(k, 1))()
    check(L.tdr_batch_pose(arr, k, out, _vp(stream) if stream else None))
    mean = np.array([list(o.mean) for o in out[:k]], np.float32).reshape(k, 4)
    cov = np.array([list(o.cov) for o in out[:k]], np.float32).reshape(k, 4, 4)
    return mean, cov, np.array([o.scale for o in out[:k]], np.float32), np.array([o.n for o in out[:k]], np.int64)


def scan_pictures_batch(renderers, unflatten, lut_bgr, stream=None):
    """Renderer.picture of every renderer in one tdr_batch_scan_pictures (one launch, one copy, one wait): a
    (k, cols, rows, 3) uint8 array.  The renders must share one shape."""
    L = _lib.load()
    k = len(renderers)
    shape = renderers[0]._shape if k and renderers[0]._shape else (0, 0, 0)
    unf, lut = _picture_tables(unflatten, lut_bgr, shape[0])
    arr = (_vp * max(k, 1))(*[r.h for r in renderers])
    out = np.zeros((k, shape[2], shape[1], 3), np.uint8)
    check(L.tdr_batch_scan_pictures(arr, k, _ptr(unf), _ptr(lut), _ptr(out) if out.size else None,
                                    _vp(stream) if stream else None))
    return out


def visualize_batch(filters, pub_scale, arrows=None, stream=None):
    """FilterHandle.visualize of every filter in one tdr_batch_visualize: a list of (out_h, out_w, 3) uint8 arrays.
    arrows: None, or per filter None / an (m, 4) integer list."""
    L = _lib.load()
    k = len(filters)
    arrows = [None] * k if arrows is None else list(arrows)
    if len(arrows) != k:
        raise ValueError("visualize_batch: one arrow list (or None) per filter")
    arr = (_vp * max(k, 1))(*[f.h for f in filters])
    req = (VizRequestC * max(k, 1))()
    keep = []
    for i, a in enumerate(arrows):
        if a is not None and len(a):
            a = np.ascontiguousarray(a, np.int32).reshape(-1, 4)
            keep.append(a)
            req[i].extra_arrows, req[i].m = a.ctypes.data, len(a)
    check(L.tdr_batch_visualize(arr, k, C.c_float(pub_scale), req, _vp(stream) if stream else None))   # the sizes
    outs = [np.zeros((req[i].out_h, req[i].out_w, 3), np.uint8) for i in range(k)]
    for i, o in enumerate(outs):
        req[i].out_bgr_host, req[i].capacity = o.ctypes.data, o.size
    check(L.tdr_batch_visualize(arr, k, C.c_float(pub_scale), req, _vp(stream) if stream else None))
    return outs


CLASSIC_PALETTE = ((0, 0, 255), (0, 255, 0), (255, 0, 0))   # one robot's colours in tdr_filter_visualize: arrows, dots, estimate


def visualize_fleet(filters, pub_scale, palette, arrows=None, stream=None):
    """The fleet picture (tdr_batch_visualize_fleet): every filter's cloud in ONE (out_h, out_w, 3) uint8 image over the
    background their map holds (MapHandle.set_viz_background).  palette: (k, 3, 3) uint8, per robot the BGR of its
    arrows, its border dots and its estimate; arrows: None or one (m, 4) integer list for the image."""
    L = _lib.load()
    k = len(filters)
    pal = np.ascontiguousarray(palette, np.uint8)
    if pal.size != 9 * k:
        raise ValueError("visualize_fleet: the palette is (k, 3, 3) BGR bytes")
    arr = None if arrows is None or len(arrows) == 0 else np.ascontiguousarray(arrows, np.int32).reshape(-1, 4)
    m, ap = (0, None) if arr is None else (len(arr), _ptr(arr))
    hs = (_vp * max(k, 1))(*[f.h for f in filters])
    st = _vp(stream) if stream else None
    oh, ow = C.c_int(), C.c_int()
    check(L.tdr_batch_visualize_fleet(hs, k, C.c_float(pub_scale), _ptr(pal), ap, m, None, 0, C.byref(oh), C.byref(ow), st))
    out = np.zeros((oh.value, ow.value, 3), np.uint8)
    check(L.tdr_batch_visualize_fleet(hs, k, C.c_float(pub_scale), _ptr(pal), ap, m, _ptr(out), out.size, C.byref(oh),
                                      C.byref(ow), st))
    return out


class _PoseView:
    """What TopDownRenderCore.publishPoseEst asks of its filter, answered from one robot's share of a pose_batch; a
    freezeScale goes to the filter, and the scale is read from it again afterwards (the freeze changes it)."""

    def __init__(self, handle, mean, cov, scale, n):
        self.h, self.mean, self.cov, self.scale_, self.n, self.froze = handle, mean, cov, scale, n, False

    def computeMeanCov(self):
        return self.cov

    def meanLikelihood(self):
        return self.mean

    def scale(self):
        return self.h.scale() if self.froze else self.scale_

    def numParticles(self):
        return int(self.n)

    def isScaleFrozen(self):
        return self.h.is_scale_frozen()

    def freezeScale(self):
        self.h.freeze_scale()
        self.froze = True


class HandleView(_PoseView):
    """The same questions asked of a FilterHandle directly (the standalone form of one robot's loop)."""

    def __init__(self, handle):
        st, cov = handle.mean_cov()
        super().__init__(handle, st, cov, handle.scale(), handle.num_particles())


class LoopBatch:
    """The node's per-scan loop (TopDownRenderCore.takeStep: render at the robot's range scale, propagate + update,
    publishPoseEst) for many robots on one map: tdr_batch_render_polar, tdr_batch_step, tdr_batch_pose, then each robot's
    own TopDownRenderCore.publishPoseEst over the read-back statistics — the range-scale, freeze and convergence rules
    are that method's.  filters: FilterHandles on one map; renderers: one Renderer per robot; cfgs: one CoreConfig per
    robot (or one for all)."""

    def __init__(self, filters, renderers, cfgs, ang_res, ncls, nb, nr):
        from .top_down_render_core import CoreConfig, TopDownRenderCore
        k = len(filters)
        if len(renderers) != k:
            raise ValueError("LoopBatch: one renderer per filter")
        cfgs = list(cfgs) if isinstance(cfgs, (list, tuple)) else [cfgs or CoreConfig()] * k
        self.filters, self.renderers = list(filters), list(renderers)
        for i, c in enumerate(cfgs):
            c.check()
            if c.recovery_every > 0 and c.recovery_candidates > 1:
                raise ValueError(f"LoopBatch: robot {i} has recovery_candidates = {c.recovery_candidates}: sensor resetting is "
                                 "not built for a batch (tdr_batch_inject is the plain injection)")
        self.cores = [TopDownRenderCore(c) for c in cfgs]
        self.ang_res, self.ncls, self.nb, self.nr = float(ang_res), int(ncls), int(nb), int(nr)
        self.stats = (0, 0)

    def take_step(self, clouds, priors, n_targets=None, stream=None):
        """clouds[k] = (pts, stride, ioff); priors[k] = (tx, ty, yaw).  Returns one PoseEst per robot."""
        res = [np.float32(c.current_range_scale_) for c in self.cores]
        for c, r in zip(self.cores, res):
            c.last_res_ = r
        render_batch(self.renderers, clouds, [float(r) for r in res], self.ang_res, self.ncls, self.nb, self.nr, stream)
        if n_targets is None and any(c.cfg.gmm_every > 0 for c in self.cores):   # :151-157 from each robot's last fit
            n_targets = [f.adaptive_count() if c.cfg.gmm_every > 0 else -1 for c, f in zip(self.cores, self.filters)]
        if n_targets is None and any(c.kld_target_ is not None for c in self.cores):   # ... or from its last bin count
            n_targets = [-1 if c.kld_target_ is None else c.kld_target_ for c in self.cores]
        self.stats = step_batch(self.filters, self.renderers, [float(r) for r in res], priors, n_targets, stream)
        mean, cov, scale, n = pose_batch(self.filters, stream)
        out, due, kld_due = [], [], {}
        for i, (c, f) in enumerate(zip(self.cores, self.filters)):
            c.filter_ = _PoseView(f, mean[i], cov[i], float(scale[i]), n[i])
            out.append(c.publishPoseEst())
            c.filter_ = None
            if c.countStepAndGmmDue():
                due.append(f)
            if c.countStepAndKldDue():   # (cores with equal parameters share a launch)
                kld_due.setdefault(bytes(kld_params_c(c.cfg.kld)), []).append(i)
        if due:   # one mixture fit for the robots whose step is due (CoreConfig.gmm_every)
            compute_gmm_batch(due, stream)
        for ids in kld_due.values():   # one bin count for the robots whose step is due (CoreConfig.kld_every)
            _, _, target = kld_count([self.filters[i] for i in ids], self.cores[ids[0]].cfg.kld, stream)
            for i, t in zip(ids, target):
                self.cores[i].kld_target_ = int(t)
        # recovery (CoreConfig.recovery_every): each due robot's tracker takes its update's mean raw weight; the robots it
        # asks an injection for share one launch per heading mode
        inj = {}
        for i, (c, f) in enumerate(zip(self.cores, self.filters)):
            if not c.countStepAndRecoveryDue():
                continue
            rp = recovery_params_c(c.cfg.recovery)
            nxt = _lib.RecoveryStateC(c.recovery_state_.w_slow, c.recovery_state_.w_fast)
            p = float(self.filters[i].L.tdr_recovery_track_host(C.byref(nxt), C.c_double(float(f.weight_stats()[2])), C.byref(rp)))
            c.last_recovery_ = (p, 0)
            if p > 0.0:
                inj.setdefault(rp.heading_mode, []).append((i, p, rp.seed))
                f.L.tdr_recovery_reset_host(C.byref(nxt))
            c.recovery_state_ = nxt
        for mode, items in inj.items():
            counts = inject([self.filters[i] for i, _, _ in items], [p for _, p, _ in items], mode,
                            [s for _, _, s in items], stream=stream)
            for (i, p, _), cnt in zip(items, counts):
                self.cores[i].last_recovery_ = (p, int(cnt))
        return out

    def scan_pictures(self, unflatten, lut_bgr, stream=None):
        """The robots' scan pictures after a take_step (publishSemanticTopDown of each): (k, nr, nb, 3) uint8."""
        return scan_pictures_batch(self.renderers, unflatten, lut_bgr, stream)

    def particle_pictures(self, pub_scale, arrows=None, stream=None):
        """The robots' particle pictures after a take_step, each over its filter's own background
        (FilterHandle.set_viz_background): a list of (out_h, out_w, 3) uint8 arrays."""
        return visualize_batch(self.filters, pub_scale, arrows, stream)

    def fleet_picture(self, pub_scale, palette, arrows=None, stream=None):
        """All robots after a take_step in one image over the map's background (MapHandle.set_viz_background):
        visualize_fleet of the loop's filters."""
        return visualize_fleet(self.filters, pub_scale, palette, arrows, stream)
