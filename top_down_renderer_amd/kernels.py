"""HipKernels: the one product implementation of the kernel interface the host classes use — thin wrappers that
hand torch-owned device memory and the current HIP stream to the stateless launchers of libtdr_hip.so
(include/tdr.h).  PyTorch is plumbing here (device memory, streams); every computation is a hand-written HIP kernel.

There is deliberately no CPU implementation in the product: constructing HipKernels without the built extension or
without a GPU raises.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import FilterParamsC, MapDescC, check


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class ScoreCtx:
    """Owner of a tdr_score_ctx (include/tdr.h): one per filter."""

    def __init__(self, lib, handle):
        self.lib, self.handle = lib, handle

    def span(self):
        return float(self.lib.tdr_score_ctx_span(self.handle))

    def trial_calls(self):
        return int(self.lib.tdr_score_ctx_trial_calls(self.handle))

    def __del__(self):
        try:
            if self.handle:
                self.lib.tdr_score_ctx_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class DevPtr:
    """A raw device pointer the library handed out, passed on like a tensor."""

    def __init__(self, addr):
        self.addr = addr

    def data_ptr(self):
        return self.addr


class RngPipe:
    """Owner of a tdr_rng_pipe (include/tdr.h)."""

    def __init__(self, kernels, handle):
        self.k, self.lib, self.handle = kernels, kernels.lib, handle

    def on_device(self):
        return bool(self.lib.tdr_rng_pipe_on_device(self.handle))

    def from_host(self, rng):
        check(self.lib.tdr_rng_pipe_from_host(self.handle, rng, self.k.stream()))

    def to_host(self, rng):
        check(self.lib.tdr_rng_pipe_to_host(self.handle, rng, self.k.stream()))

    def normals(self, n, lo, hi, scale_freeze):
        z = C.c_void_p(0)
        check(self.lib.tdr_rng_pipe_normals(self.handle, n, lo, hi, int(scale_freeze), C.byref(z), self.k.stream()))
        return DevPtr(z.value)

    def uniform(self):
        u = C.c_void_p(0)
        check(self.lib.tdr_rng_pipe_uniform(self.handle, C.byref(u), self.k.stream()))
        return DevPtr(u.value)

    def init_particles(self, dmap, fp, max_num, lo, hi, st):
        """initializeParticles' particle loop on the pipe's state (tdr_rng_pipe_init_particles): particles [lo, hi) into
        the SoA planes st; returns the count the loop keeps."""
        n = C.c_int64(0)
        ws = self.k.empty((int(self.lib.tdr_init_workspace_bytes()),), torch.uint8)
        check(self.lib.tdr_rng_pipe_init_particles(self.handle, C.byref(dmap.desc), C.byref(fp), max_num, lo, hi, _ptr(st),
                                                   st.shape[1], C.byref(n), _ptr(ws), self.k.stream()))
        return n.value

    def __del__(self):
        try:
            if self.handle:
                self.lib.tdr_rng_pipe_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class IngestState:
    """What make_map_from_labels(keep_ingest=True) keeps for incremental updates: the device image and LUT, the host LUT,
    the ingest workspace (class words + column distances), the image shape, the class count and the resolution."""

    def __init__(self, img, lut_d, lut, ws, shape, ncls, resolution):
        self.img, self.lut_d, self.lut, self.ws = img, lut_d, lut, ws
        self.shape, self.ncls, self.resolution = tuple(shape), int(ncls), float(resolution)


class DeviceMap:
    """Device-resident interleaved map (tdr_map_desc) + the polar sampling table."""

    def __init__(self, rec, ncls, rows, cols, resolution):
        self.rec, self.ncls, self.rows, self.cols, self.resolution = rec, ncls, rows, cols, float(resolution)
        self.rec_floats = _lib.load().tdr_rec_floats(ncls)
        self.desc = MapDescC(rec.data_ptr(), ncls, rows, cols, self.rec_floats, self.resolution)
        self.tab = None       # device (P,2) f32
        self.tab_host = None  # numpy (P,2) f32
        self.fac = None       # device (2 nb + nr,) f32: the table's factors (tdr_polar_factors_host)
        self.nb = self.nr = 0
        self.ang_res = 0.0
        self.crec = self.dict = None   # compact form of the records (tdr_k_compact_map), when the map has one
        self.rec16 = None              # scratch of the 40-rotation search (tdr_map_desc.rec16), allocated on first use
        self.use_rec16 = True          # False: the search splits the f32 records on the fly (A/B, tests)
        self.ingest = None             # IngestState of a label-image map kept for incremental updates
        self.counts = None             # the dictionary's occurrence counts (tdr_k_map_dict_counts), current if counts_ok
        self.counts_ok = False
        self.incr_ws = None
        self.road = None               # the road list (HipKernels.road_cells), built on first use; a record write drops it

    def init_scratch(self, kernels):
        """Gives the descriptor the scratch the matrix-core init search writes its pre-split f16 records to."""
        if not self.use_rec16:
            self.desc.rec16 = None
            return
        if self.rec16 is None:
            nbytes = int(kernels.lib.tdr_map_rec16_bytes(self.ncls, self.rows, self.cols))
            if nbytes == 0:
                return
            self.rec16 = kernels.empty((nbytes,), torch.uint8)
        self.desc.rec16 = self.rec16.data_ptr()

    def geo_map(self, kernels, constant_one=False):
        """geo_maps_[0..1] as a 2-class DeviceMap (tdr_k_geo_map_from_map): distance to the nearest cell without / with
        a geometric class, derived from the class records; constant_one: what the reference's updateMap path leaves."""
        key = bool(constant_one)
        if getattr(self, "_geo", None) is None or self._geo[0] != key:
            lib = kernels.lib
            rec = kernels.empty((int(lib.tdr_map_rec_floats_total(2, self.rows, self.cols)),))
            ws = kernels.empty((int(lib.tdr_map_ingest_workspace_bytes(2, self.rows, self.cols)),), torch.uint8)
            check(lib.tdr_k_geo_map_from_map(C.byref(self.desc), int(key), _ptr(rec), _ptr(ws), kernels.stream()))
            kernels.synchronize()
            g = DeviceMap(rec, 2, self.rows, self.cols, self.resolution)
            g.tab, g.tab_host, g.nb, g.nr, g.ang_res = self.tab, self.tab_host, self.nb, self.nr, self.ang_res
            self._geo = (key, g)
        g = self._geo[1]
        g.tab, g.tab_host, g.nb, g.nr, g.ang_res = self.tab, self.tab_host, self.nb, self.nr, self.ang_res
        return g

    def compact(self, kernels):
        """Builds the compact records (csrc/tdr_cmap.hip): 10-bit dictionary indices instead of floats, exact by
        construction; read by scoring waves whose particles are spread over the map.  No-op for maps without one."""
        lib = kernels.lib
        nw = int(lib.tdr_cmap_words_total(self.ncls, self.rows, self.cols))
        if nw == 0:
            return False
        crec = kernels.empty((nw,), torch.int32)
        dic = kernels.empty((4096,))                    # TDR_CMAP_WIDE_MAX_DICT
        ws = kernels.empty((16384 * 4 + 16384 * 2 + 256,), torch.uint8)   # TDR_CMAP_WORKSPACE_BYTES
        check(lib.tdr_k_compact_map(C.byref(self.desc), _ptr(crec), _ptr(dic), _ptr(ws), kernels.stream()))
        if not self.desc.cwords and self.desc.dict_n < 0:
            # more than 1024 distinct distance values (a fine map resolution): the wide form, 16-bit fields
            crec = kernels.empty((int(lib.tdr_cmap_wide_words_total(self.ncls, self.rows, self.cols)),), torch.int32)
            check(lib.tdr_k_compact_map_wide(C.byref(self.desc), _ptr(crec), _ptr(dic), _ptr(ws), kernels.stream()))
        if self.desc.cwords:
            self.crec, self.dict = crec, dic            # keep the device memory alive with the descriptor
        else:
            self.desc.dict_n = 0
        return bool(self.desc.cwords)


def svg_parse(path):
    """tdr_svg_parse_host (host only, no GPU): the polygons TopDownMap::loadSvg keeps of an SVG.  Returns
    (size float32[2] = the image's float width / height, keys uint32[P] (_lib.TDR_SVG_NO_KEY: gradient),
    offs int64[P + 1], verts float32[V, 2] = (x, height - y))."""
    lib = _lib.load()
    size = np.zeros(2, np.float32)
    n_poly, n_vert = C.c_int64(0), C.c_int64(0)
    check(lib.tdr_svg_parse_host(str(path).encode(), size.ctypes.data_as(C.c_void_p), C.byref(n_poly), C.byref(n_vert),
                                 None, None, None))
    keys = np.zeros(max(n_poly.value, 1), np.uint32)
    offs = np.zeros(n_poly.value + 1, np.int64)
    verts = np.zeros((max(n_vert.value, 1), 2), np.float32)
    check(lib.tdr_svg_parse_host(str(path).encode(), size.ctypes.data_as(C.c_void_p), C.byref(n_poly), C.byref(n_vert),
                                 keys.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p),
                                 verts.ctypes.data_as(C.c_void_p)))
    return size, keys[:n_poly.value], offs, verts[:n_vert.value]


def png_read_color(path):
    """tdr_png_read_color_host (host only, no GPU): the BGR8 image cv::imread(path) gives for a PNG, (H, W, 3) uint8,
    row 0 = top, channels B, G, R."""
    lib = _lib.load()
    w, h = C.c_int(0), C.c_int(0)
    rc = lib.tdr_png_read_color_host(str(path).encode(), None, 0, C.byref(w), C.byref(h))   # size query
    if w.value < 1 or h.value < 1:
        check(rc)
    out = np.empty((h.value, w.value, 3), np.uint8)
    check(lib.tdr_png_read_color_host(str(path).encode(), out.ctypes.data_as(C.c_void_p), out.size, C.byref(w),
                                      C.byref(h)))
    return out


def viz_arrow_host(dx, dy):
    """Host: the three segments {x1, y1, x2, y2} of Arrow(-(dx, dy), (dx, dy)) (include/tdr.h, "the particle picture")."""
    segs = np.zeros((3, 4), np.int32)
    check(_lib.load().tdr_viz_arrow_host(int(dx), int(dy), segs.ctypes.data_as(C.c_void_p)))
    return segs


def viz_overlay_host(means, covs, best, arrows, H):
    """Host: the overlay of the particle picture as int32 segments {x1, y1, x2, y2, plane}.  means (k, 3), covs (k, 3, 3):
    the mixture; best: {x, y, theta} of the max-likelihood state or None; arrows: (m, 4) caller's arrows or None."""
    means = np.ascontiguousarray(means, np.float32).reshape(-1, 3)
    covs = np.ascontiguousarray(covs, np.float32).reshape(-1, 9)
    arrows = np.zeros((0, 4), np.int32) if arrows is None else np.ascontiguousarray(arrows, np.int32).reshape(-1, 4)
    best_p = None if best is None else np.ascontiguousarray(best, np.float32)[:3].copy()
    k, m = len(means), len(arrows)
    cap = 75 * k + 3 + 3 * m   # TDR_VIZ_MAX_SEGS
    segs = np.zeros((cap, 5), np.int32)
    n = C.c_int(0)
    check(_lib.load().tdr_viz_overlay_host(
        means.ctypes.data_as(C.c_void_p) if k else None, covs.ctypes.data_as(C.c_void_p) if k else None, k,
        None if best_p is None else best_p.ctypes.data_as(C.c_void_p),
        arrows.ctypes.data_as(C.c_void_p) if m else None, m, int(H), segs.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
    return segs[: n.value].copy()


class HipKernels:
    name = "hip"

    def __init__(self, device=None):
        self.lib = _lib.load()
        if not torch.cuda.is_available() or self.lib.tdr_device_count() < 1:
            raise _lib.TdrError("no HIP device visible: the MI355X path cannot run (there is no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._ws = None
        self._init_ws = None   # the Cartesian heading search (score_cart_init): freed with the kernels object
        self._pws = None
        self._rws = None

    # ---- plumbing -------------------------------------------------------------------------------------------
    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def empty(self, shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def zeros(self, shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device=self.device)

    def to_device(self, array):
        return torch.from_numpy(np.ascontiguousarray(array)).to(self.device)

    def synchronize(self):
        torch.cuda.synchronize(self.device)

    def read_device_floats(self, dev, n):
        """n floats behind a device pointer the library handed out (synchronises)."""
        if getattr(self, "_hip", None) is None:
            self._hip = C.CDLL("libamdhip64.so")
        self.synchronize()
        out = np.zeros(n, np.float32)
        rc = self._hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(dev.data_ptr()), C.c_size_t(4 * n), 2)
        if rc != 0:
            raise _lib.TdrError(f"hipMemcpy device -> host failed ({rc})")
        return out

    # ---- map ------------------------------------------------------------------------------------------------
    def make_map(self, class_maps, class_mask, resolution):
        """class_maps (ncls,H,W) f32 indexed [cls,row,col]; class_mask (H,W) u8.  Uploaded in the reference's
        column-major per-class layout and interleaved on the device by tdr_k_pack_map."""
        ncls, H, W = class_maps.shape
        maps_cm = self.to_device(np.ascontiguousarray(np.transpose(class_maps, (0, 2, 1)), np.float32))
        mask_cm = self.to_device(np.ascontiguousarray(class_mask.T, np.uint8))
        rec = self.empty((int(self.lib.tdr_map_rec_floats_total(ncls, H, W)),))
        check(self.lib.tdr_k_pack_map(_ptr(maps_cm), _ptr(mask_cm), ncls, H, W, _ptr(rec), self.stream()))
        self.synchronize()
        del maps_cm, mask_cm
        m = DeviceMap(rec, ncls, H, W, resolution)
        m.compact(self)
        return m

    def make_map_from_labels(self, label_img, flatten_lut, ncls, resolution, keep_ingest=False):
        """label_img: (img_h, img_w) uint8 class-index image (cv::Mat layout, row 0 = top).  Runs
        loadCompressedRasterMap + computeDists on the device (tdr_k_map_from_labels).  keep_ingest: the map keeps the
        image, the LUT and the ingest workspace (class words, column distances) for update_map_from_labels."""
        label_img = np.ascontiguousarray(label_img, np.uint8)
        img_h, img_w = label_img.shape
        rows, cols = C.c_int(0), C.c_int(0)
        check(self.lib.tdr_map_ingest_shape(img_h, img_w, C.c_float(resolution), C.byref(rows), C.byref(cols)))
        rows, cols = rows.value, cols.value
        lut = np.ascontiguousarray(flatten_lut, np.int32).ravel()
        img_d, lut_d = self.to_device(label_img), self.to_device(lut)
        rec = self.empty((int(self.lib.tdr_map_rec_floats_total(ncls, rows, cols)),))
        ws = self.empty((int(self.lib.tdr_map_ingest_workspace_bytes(ncls, rows, cols)),), torch.uint8)
        check(self.lib.tdr_k_map_from_labels(_ptr(img_d), img_h, img_w, _ptr(lut_d), len(lut), ncls,
                                             C.c_float(resolution), _ptr(rec), _ptr(ws), self.stream()))
        self.synchronize()
        m = DeviceMap(rec, ncls, rows, cols, resolution)
        m.compact(self)
        if keep_ingest:
            m.ingest = IngestState(img_d, lut_d, lut, ws, (img_h, img_w), ncls, float(resolution))
        return m

    def update_map_from_labels(self, m, label_img, max_cells=-1):
        """The incremental ingest (tdr_k_map_update_labels) of a new label image into a DeviceMap built by
        make_map_from_labels(keep_ingest=True) from an image of the same shape, LUT and class count: only the cells
        within R = ceil(50 / resolution) of a changed cell are rebuilt; the compact form is refreshed in place, or built
        anew when its dictionary changes.  Returns (changed_cells, affected tiles) — None, with nothing changed, when the
        affected tiles hold more than max_cells cells (>= 0)."""
        ing, lib = m.ingest, self.lib
        label_img = np.ascontiguousarray(label_img, np.uint8)
        if label_img.shape != ing.shape:
            raise ValueError("update_map_from_labels: the image shape differs from the map's last image")
        ing.img.copy_(torch.from_numpy(label_img))
        if m.desc.cwords and not m.counts_ok:
            if m.counts is None:
                m.counts = self.empty((4096,), torch.int32)   # TDR_CMAP_WIDE_MAX_DICT
            check(lib.tdr_k_map_dict_counts(C.byref(m.desc), _ptr(m.counts), self.stream()))
            m.counts_ok = True
        if m.incr_ws is None:
            m.incr_ws = self.empty((int(lib.tdr_map_incr_workspace_bytes(m.rows, m.cols)),), torch.uint8)
        tiles = np.zeros(max(1, int(lib.tdr_map_incr_tiles(m.rows, m.cols))), np.int32)
        n_tiles, changed, compact_ok = C.c_int(0), C.c_int64(0), C.c_int(0)
        check(lib.tdr_k_map_update_labels(_ptr(ing.img), ing.shape[0], ing.shape[1], _ptr(ing.lut_d), len(ing.lut),
                                          C.byref(m.desc), _ptr(ing.ws), _ptr(m.counts) if m.desc.cwords else None,
                                          int(max_cells), _ptr(m.incr_ws), tiles.ctypes.data_as(C.c_void_p),
                                          C.byref(n_tiles), C.byref(changed), C.byref(compact_ok), self.stream()))
        if n_tiles.value < 0:
            return None
        m.road = None   # the records changed
        if not compact_ok.value:
            m.counts_ok = False
            m.compact(self)
        return changed.value, tiles[:n_tiles.value].copy()

    def gather_tiles(self, m, tiles):
        """The cells of the listed tiles (tdr_k_map_gather_tiles): (n, ncls, T, T) float32 indexed [tile, class, column,
        row] like class_maps_, and (n, T, T) uint8 masks (1 = unknown), T = TDR_MAP_INCR_TILE."""
        T = 32
        n = len(tiles)
        maps = self.zeros((max(n, 1), m.ncls, T, T))
        mask = self.zeros((max(n, 1), T, T), torch.uint8)
        if n:
            t_d = self.to_device(np.ascontiguousarray(tiles, np.int32))
            check(self.lib.tdr_k_map_gather_tiles(_ptr(m.rec), m.ncls, m.rows, m.cols, _ptr(t_d), n, _ptr(maps), _ptr(mask),
                                                  self.stream()))
        return maps[:n].cpu().numpy(), mask[:n].cpu().numpy()

    def make_map_from_rasters(self, planes, resolution):
        """planes: (ncls, rows, cols) uint8, the class<i>.png images of a raster cache as stored (row 0 = top).  Runs
        loadRasterizedMaps' flip + computeDists on the device (tdr_k_map_from_rasters)."""
        planes = np.ascontiguousarray(planes, np.uint8)
        ncls, rows, cols = planes.shape
        pl_d = self.to_device(planes.reshape(-1))
        rec = self.empty((int(self.lib.tdr_map_rec_floats_total(ncls, rows, cols)),))
        ws = self.empty((int(self.lib.tdr_map_ingest_workspace_bytes(ncls, rows, cols)),), torch.uint8)
        check(self.lib.tdr_k_map_from_rasters(_ptr(pl_d), ncls, rows, cols, C.c_float(resolution), _ptr(rec), _ptr(ws),
                                              self.stream()))
        self.synchronize()
        m = DeviceMap(rec, ncls, rows, cols, resolution)
        m.compact(self)
        return m

    def make_map_from_color(self, bgr, fill_keys, flatten_lut, ncls, resolution):
        """bgr: (img_h, img_w, 3) uint8 image in cv::imread's layout.  Runs color2Ind + loadCompressedRasterMap +
        computeDists on the device (tdr_k_map_from_color); fill_keys[i] = the key of LUT index i."""
        bgr = np.ascontiguousarray(bgr, np.uint8)
        img_h, img_w = bgr.shape[:2]
        rows, cols = C.c_int(0), C.c_int(0)
        check(self.lib.tdr_map_ingest_shape(img_h, img_w, C.c_float(resolution), C.byref(rows), C.byref(cols)))
        rows, cols = rows.value, cols.value
        keys = np.ascontiguousarray(fill_keys, np.uint32).ravel()
        lut = np.ascontiguousarray(flatten_lut, np.int32).ravel()
        if len(keys) < len(lut):
            raise ValueError("one fill key per flatten_lut entry is needed")
        img_d = self.to_device(bgr)
        rec = self.empty((int(self.lib.tdr_map_rec_floats_total(ncls, rows, cols)),))
        ws = self.empty((int(self.lib.tdr_map_ingest_workspace_bytes(ncls, rows, cols)),), torch.uint8)
        check(self.lib.tdr_k_map_from_color(_ptr(img_d), img_h, img_w, keys.ctypes.data_as(C.c_void_p),
                                            lut.ctypes.data_as(C.c_void_p), len(lut), ncls, C.c_float(resolution),
                                            _ptr(rec), _ptr(ws), self.stream()))
        self.synchronize()
        m = DeviceMap(rec, ncls, rows, cols, resolution)
        m.compact(self)
        return m

    def color_index(self, bgr, fill_keys):
        """color2Ind on the device (tdr_k_color_index): (H, W, 3) uint8 BGR -> (H, W) uint8 LUT indices, 255 where no
        key matches.  bgr may be a numpy array or a cuda uint8 tensor; a tensor gives a tensor."""
        keys = np.ascontiguousarray(fill_keys, np.uint32).ravel()
        on_dev = isinstance(bgr, torch.Tensor)
        img_d = bgr.contiguous() if on_dev else self.to_device(np.ascontiguousarray(bgr, np.uint8))
        if img_d.dtype != torch.uint8 or img_d.dim() != 3 or img_d.shape[2] != 3:
            raise ValueError("color_index needs an (H, W, 3) uint8 image")
        out = self.empty(tuple(img_d.shape[:2]), torch.uint8)
        check(self.lib.tdr_k_color_index(_ptr(img_d), img_d.shape[0], img_d.shape[1], keys.ctypes.data_as(C.c_void_p),
                                         len(keys), _ptr(out), self.stream()))
        if on_dev:
            return out
        return out.cpu().numpy()

    def map_load_color_image(self, handle, bgr, fill_keys, flatten_lut, ncls, resolution, center=(0, 0)):
        """tdr_map_load_color_image: the reference constructor's colour-map branch on a tdr_map handle, from a host
        (H, W, 3) uint8 BGR image."""
        bgr = np.ascontiguousarray(bgr, np.uint8)
        keys = np.ascontiguousarray(fill_keys, np.uint32)
        lut = np.ascontiguousarray(flatten_lut, np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
        check(self.lib.tdr_map_load_color_image(handle, vp(bgr), bgr.shape[0], bgr.shape[1], vp(keys), vp(lut), len(lut),
                                                int(ncls), C.c_float(resolution), int(center[0]), int(center[1])))

    def map_load_color_png(self, handle, path, fill_keys, flatten_lut, ncls, resolution, center=(0, 0)):
        """tdr_map_load_color_png: read the PNG (host), then tdr_map_load_color_image's path."""
        keys = np.ascontiguousarray(fill_keys, np.uint32)
        lut = np.ascontiguousarray(flatten_lut, np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
        check(self.lib.tdr_map_load_color_png(handle, str(path).encode(), vp(keys), vp(lut), len(lut), int(ncls),
                                              C.c_float(resolution), int(center[0]), int(center[1])))

    def map_load_polygons(self, handle, verts, offs, cls, width, height, ncls, exclusive, resolution, center=(0, 0),
                          want_planes=True):
        """tdr_map_load_polygons on a tdr_map handle: getRasterMap + getClasses of the polygons (vertex (x, y) pairs
        verts[offs[p]:offs[p+1]], class cls[p]) on the device, then the ingest.  Returns the class planes before the
        distance transform, (ncls, cols, rows) uint8 column-major (0 inside, 1 elsewhere), or None."""
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 2)
        offs = np.ascontiguousarray(offs, np.int64)
        cls = np.ascontiguousarray(cls, np.int32)
        excl = np.ascontiguousarray(exclusive, np.int32)
        rows, cols = int(np.float32(height) / np.float32(resolution)), int(np.float32(width) / np.float32(resolution))
        planes = np.empty((ncls, cols, rows), np.uint8) if want_planes else None
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        check(self.lib.tdr_map_load_polygons(handle, vp(verts), offs.ctypes.data_as(C.c_void_p), vp(cls), len(cls),
                                             int(width), int(height), int(ncls), vp(excl), len(excl),
                                             C.c_float(resolution), int(center[0]), int(center[1]), vp(planes)))
        return planes

    def polygon_planes(self, verts, offs, cls, width, height, ncls, exclusive, resolution):
        """tdr_polygon_planes: the fill alone (getRasterMap + getClasses on the device, no ingest).  Returns the class
        planes (ncls, cols, rows) uint8 column-major (0 inside, 1 elsewhere)."""
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 2)
        offs = np.ascontiguousarray(offs, np.int64)
        cls = np.ascontiguousarray(cls, np.int32)
        excl = np.ascontiguousarray(exclusive, np.int32)
        rows, cols = int(np.float32(height) / np.float32(resolution)), int(np.float32(width) / np.float32(resolution))
        planes = np.empty((ncls, max(cols, 0), max(rows, 0)), np.uint8)
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
        check(self.lib.tdr_polygon_planes(vp(verts), offs.ctypes.data_as(C.c_void_p), vp(cls), len(cls), int(width),
                                          int(height), int(ncls), vp(excl), len(excl), C.c_float(resolution),
                                          planes.ctypes.data_as(C.c_void_p)))
        return planes

    def map_load_svg(self, handle, path, fill_keys, flatten_lut, ncls, exclusive, resolution, center=(0, 0)):
        """tdr_map_load_svg: the reference constructor's SVG branch on a tdr_map handle."""
        keys = np.ascontiguousarray(fill_keys, np.uint32)
        lut = np.ascontiguousarray(flatten_lut, np.int32)
        excl = np.ascontiguousarray(exclusive, np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
        check(self.lib.tdr_map_load_svg(handle, str(path).encode(), vp(keys), vp(lut), len(lut), int(ncls), vp(excl),
                                        len(excl), C.c_float(resolution), int(center[0]), int(center[1])))

    def png_read_gray8(self, path):
        w, h = C.c_int(0), C.c_int(0)
        rc = self.lib.tdr_png_read_gray8_host(str(path).encode(), None, 0, C.byref(w), C.byref(h))   # size query
        if w.value < 1 or h.value < 1:
            check(rc)
        out = np.empty((h.value, w.value), np.uint8)
        check(self.lib.tdr_png_read_gray8_host(str(path).encode(), out.ctypes.data_as(C.c_void_p), out.size, C.byref(w), C.byref(h)))
        return out

    def png_write_gray8(self, path, img):
        img = np.ascontiguousarray(img, np.uint8)
        check(self.lib.tdr_png_write_gray8_host(str(path).encode(), img.ctypes.data_as(C.c_void_p), img.shape[1], img.shape[0]))

    def unpack_map(self, m):
        """Device map -> the reference's host layout: class maps (ncls, cols, rows) i.e. column-major, mask (cols, rows)."""
        maps = self.empty((m.ncls, m.cols, m.rows))
        mask = self.empty((m.cols, m.rows), torch.uint8)
        check(self.lib.tdr_k_unpack_map(_ptr(m.rec), m.ncls, m.rows, m.cols, _ptr(maps), _ptr(mask), self.stream()))
        return maps.cpu().numpy(), mask.cpu().numpy()

    def set_polar_table(self, m, nb, nr, ang_res):
        tab = np.empty((nb * nr, 2), np.float32)
        check(self.lib.tdr_polar_table_host(nb, nr, C.c_float(ang_res), C.c_float(m.resolution),
                                            tab.ctypes.data_as(C.c_void_p)))
        m.tab_host, m.tab, m.nb, m.nr, m.ang_res = tab, self.to_device(tab), nb, nr, float(ang_res)
        fac = np.empty(2 * nb + nr, np.float32)
        check(self.lib.tdr_polar_factors_host(nb, nr, C.c_float(ang_res), C.c_float(m.resolution),
                                              fac.ctypes.data_as(C.c_void_p)))
        m.fac = self.to_device(fac)

    # ---- raster ---------------------------------------------------------------------------------------------
    def _raster_workspace(self, n):
        need = int(self.lib.tdr_raster_workspace_bytes(n))
        if self._rws is None or self._rws.numel() < need:
            self._rws = self.empty((max(need, 4),), torch.uint8)
        return self._rws

    def raster_polar(self, pts, n, stride, ioff, res, ang_res, lut, ncls, nb, nr, want_img=True):
        img = self.empty((ncls, nb * nr)) if want_img else None
        pk = self.empty((nr * nb * self.lib.tdr_rec_floats(ncls),))
        check(self.lib.tdr_k_raster_polar(_ptr(pts), stride, ioff, n, C.c_float(res), C.c_float(ang_res), _ptr(lut),
                                          ncls, nb, nr, _ptr(img), _ptr(pk), _ptr(self._raster_workspace(n)),
                                          self.stream()))
        return img, pk

    def raster_cart(self, pts, n, stride, ioff, res, lut, ncls, rows, cols, want_img=True):
        img = self.empty((ncls, rows * cols)) if want_img else None
        pk = self.empty((rows * cols * self.lib.tdr_rec_floats(ncls),))
        check(self.lib.tdr_k_raster_cart(_ptr(pts), stride, ioff, n, C.c_float(res), _ptr(lut), ncls, rows, cols,
                                         _ptr(img), _ptr(pk), _ptr(self._raster_workspace(n)), self.stream()))
        return img, pk

    def raster_geo(self, pts, stride, width, height, res, ang_res, rows, cols, polar):
        """renderGeometricTopDown on a device cloud (organised: element idy*width + idx): (2, rows*cols) device images."""
        img = self.empty((2, rows * cols))
        if polar:
            ws = self.empty((int(self.lib.tdr_raster_geo_workspace_bytes(max(1, width * height))),), torch.uint8)
            check(self.lib.tdr_k_raster_geo_polar(_ptr(pts), stride, width, height, C.c_float(res), C.c_float(ang_res),
                                                  rows, cols, _ptr(img), _ptr(ws), self.stream()))
        else:
            check(self.lib.tdr_k_raster_geo_cart(_ptr(pts), stride, width, height, C.c_float(res), rows, cols, _ptr(img),
                                                 self.stream()))
        return img

    # ---- getLocalMap materialised ----------------------------------------------------------------------------
    def local_map(self, m, polar, cx, cy, scale_or_rot, res, rows=None, cols=None):
        """(dists (ncls, rows*cols) float32, mask (rows*cols,) uint8) device tensors: the window of one pose
        (top_down_map_polar.cpp:21-53 / top_down_map.cpp:429-459)."""
        if polar:
            rows, cols = m.nb, m.nr
        d = self.empty((m.ncls, rows * cols))
        k = self.empty((rows * cols,), torch.uint8)
        if polar:
            check(self.lib.tdr_k_local_map_polar(C.byref(m.desc), _ptr(m.tab), rows, cols, C.c_float(cx), C.c_float(cy),
                                                 C.c_float(scale_or_rot), C.c_float(res), _ptr(d), _ptr(k), self.stream()))
        else:
            check(self.lib.tdr_k_local_map_cart(C.byref(m.desc), rows, cols, C.c_float(cx), C.c_float(cy),
                                                C.c_float(scale_or_rot), C.c_float(res), _ptr(d), _ptr(k), self.stream()))
        return d, k

    # ---- map fusion (include/tdr.h, "map fusion") -------------------------------------------------------------------
    def fuse_state(self, m):
        """(votes (ncls, rows, cols) int32 holding uint32 bits, dirty bitmap words, counters (2,) int64), all zero."""
        words = (int(self.lib.tdr_map_incr_tiles(m.rows, m.cols)) + 31) // 32
        return (self.zeros((m.ncls, m.rows, m.cols), torch.int32), self.zeros((words,), torch.int32),
                self.zeros((2,), torch.int64))

    def fuse_votes(self, m, scans, polar, poses, votes, dirty, counters):
        """One launch (tdr_k_fuse_votes_jobs) for the scans of a list: scans[k] a contiguous device tensor (ncls, cols, rows),
        which is the render layout [ncls][rows*cols] column-major; polar[k] its kind, poses[k] = (cx, cy, theta, scale, res).
        A single scan goes through tdr_k_fuse_votes."""
        tab = m.tab if m.nb > 0 else None
        args = (C.byref(m.desc), _ptr(tab) if tab is not None else None, m.nb if tab is not None else 0,
                m.nr if tab is not None else 0)
        if len(scans) == 1:
            s, (cx, cy, th, sc, res) = scans[0], poses[0]
            check(self.lib.tdr_k_fuse_votes(*args, _ptr(s), int(bool(polar[0])), s.shape[2], s.shape[1], C.c_float(cx),
                                            C.c_float(cy), C.c_float(th), C.c_float(sc), C.c_float(res), _ptr(votes),
                                            _ptr(dirty), _ptr(counters), self.stream()))
            return
        jobs = (_lib.FuseJobC * len(scans))()
        for j, s, pl, (cx, cy, th, sc, res) in zip(jobs, scans, polar, poses):
            j.scan, j.rows, j.cols, j.polar = s.data_ptr(), s.shape[2], s.shape[1], int(bool(pl))
            j.cx, j.cy, j.theta, j.scale, j.res = cx, cy, th, sc, res
        jobs_d = self.to_device(np.frombuffer(bytearray(jobs), np.uint8))
        check(self.lib.tdr_k_fuse_votes_jobs(*args, _ptr(jobs_d), len(scans), max(s.shape[1] * s.shape[2] for s in scans),
                                             _ptr(votes), _ptr(dirty), _ptr(counters), self.stream()))
        self.synchronize()   # (jobs_d is this call's)

    def fuse_labels(self, votes, img_shape, resolution, class_label, min_votes, share, base, current, tiles):
        """tdr_k_fuse_labels over the listed tiles (an int32 device tensor): `current` (img_h, img_w) uint8 is updated in
        place; returns (changed pixels, y min, x min, y max, x max)."""
        ncls, rows, cols = votes.shape
        out = self.to_device(np.asarray([0, 2 ** 31 - 1, 2 ** 31 - 1, -1, -1], np.int32))
        cl = np.ascontiguousarray(class_label, np.uint8)
        check(self.lib.tdr_k_fuse_labels(_ptr(votes), ncls, rows, cols, int(img_shape[0]), int(img_shape[1]),
                                         C.c_float(resolution), cl.ctypes.data_as(C.c_void_p), int(min_votes), int(share[0]),
                                         int(share[1]), _ptr(base), _ptr(current), _ptr(tiles), int(tiles.numel()), _ptr(out),
                                         self.stream()))
        return tuple(int(x) for x in out.cpu().numpy())

    def pack_scan(self, img, ncls, nb, nr):
        pk = self.empty((nr * nb * self.lib.tdr_rec_floats(ncls),))
        check(self.lib.tdr_k_pack_scan(_ptr(img), ncls, nb, nr, _ptr(pk), self.stream()))
        return pk

    # ---- filter ---------------------------------------------------------------------------------------------
    def _workspace(self, ncls, nb, nr, n, n_total=0):
        need = int(self.lib.tdr_score_workspace_floats(ncls, nb, nr, n, n_total))
        if self._ws is None or self._ws.numel() < need:
            self._ws = self.empty((need,))
        return self._ws

    def score_ctx_create(self):
        """A tdr_score_ctx: the span tuner of ONE caller's scoring launches and the table's factors (include/tdr.h)."""
        h = C.c_void_p(0)
        check(self.lib.tdr_score_ctx_create(C.byref(h)))
        return ScoreCtx(self.lib, h)

    def score(self, m, scan_pk, res, fp, st, n, raw_w, perm=None, init_search=False, uniform_scale=0.0, n_total=0, ctx=None):
        """n_total: particle count of the whole (possibly sharded) filter, see tdr_k_score_polar; 0 = n.
        ctx: the caller's ScoreCtx (None: the kernels of a launch one after the other on the caller's stream)."""
        ws = self._workspace(m.ncls, m.nb, m.nr, n, n_total)
        cap = st.shape[1]
        if init_search and max(n, n_total) >= int(self.lib.tdr_config_rec16_min_particles(-1)):
            m.init_scratch(self)
        if ctx is not None:   # the table as its factors (include/tdr.h): the call checks them against m.tab itself
            check(self.lib.tdr_score_ctx_set_polar_factors(ctx.handle, _ptr(getattr(m, "fac", None)), m.nb, m.nr))
        check(self.lib.tdr_k_score_polar_ctx(C.byref(m.desc), _ptr(m.tab), _ptr(scan_pk), m.nb, m.nr, C.c_float(res),
                                             C.byref(fp), _ptr(st), cap, n, n_total, _ptr(perm), C.c_float(uniform_scale),
                                             int(bool(init_search)), _ptr(raw_w), _ptr(ws),
                                             ctx.handle if ctx is not None else C.c_void_p(0), self.stream()))

    def score_geo(self, m, gm, scan_pk, geo_pk, geo_sums, res, fp, st, n, raw_w, perm=None, init_search=False,
                  uniform_scale=0.0):
        """Scoring with the geometric term (tdr_k_score_polar_geo): gm = m.geo_map(...), geo_pk = pack_scan of the two
        geometric images, geo_sums = their sums."""
        need = int(self.lib.tdr_score_geo_workspace_floats(m.ncls, m.nb, m.nr, n, 0))
        if self._ws is None or self._ws.numel() < need:
            self._ws = self.empty((need,))
        check(self.lib.tdr_k_score_polar_geo(C.byref(m.desc), C.byref(gm.desc), _ptr(m.tab), _ptr(scan_pk), _ptr(geo_pk),
                                             C.c_float(geo_sums[0]), C.c_float(geo_sums[1]), m.nb, m.nr, C.c_float(res),
                                             C.byref(fp), _ptr(st), st.shape[1], n, 0, _ptr(perm),
                                             C.c_float(uniform_scale), int(bool(init_search)), _ptr(raw_w),
                                             _ptr(self._ws), self.stream()))

    def score_cart(self, m, scan_pk, rows, cols, res, fp, st, n, raw_w, perm=None, n_total=0):
        """n_total: particle count of the whole (possibly sharded) filter, see tdr_k_score_cart; 0 = n."""
        need = int(self.lib.tdr_score_cart_workspace_floats(m.ncls, rows, cols, n, n_total))
        if self._ws is None or self._ws.numel() < need:
            self._ws = self.empty((need,))
        check(self.lib.tdr_k_score_cart(C.byref(m.desc), _ptr(scan_pk), rows, cols, C.c_float(res), C.byref(fp),
                                        _ptr(st), st.shape[1], n, n_total, _ptr(perm), _ptr(raw_w), _ptr(self._ws),
                                        self.stream()))

    def score_cart_init(self, m, scan_pk, rows, cols, res, fp, st, n, n_total=0):
        """The heading search of the Cartesian filter (tdr_k_score_cart_init): particles of st whose have_init is 0 get
        the best of the reference's 40 candidate headings and have_init = 1; the others are not touched.  Waits for the
        stream once (the number of such particles decides how many scoring launches follow)."""
        need = int(self.lib.tdr_score_cart_init_workspace_floats(m.ncls, rows, cols, n, n_total))
        if self._init_ws is None or self._init_ws.numel() < need:
            self._init_ws = self.empty((need,))
        check(self.lib.tdr_k_score_cart_init(C.byref(m.desc), _ptr(scan_pk), rows, cols, C.c_float(res), C.byref(fp),
                                             _ptr(st), st.shape[1], n, n_total, _ptr(self._init_ws), self.stream()))

    def propagate(self, st, n, last_dist, tx, ty, omega, scale_freeze, pos_cov, theta_cov, z4=None, seed=0, step=0,
                  index_base=0):
        check(self.lib.tdr_k_propagate(_ptr(st), st.shape[1], n, _ptr(last_dist), C.c_float(tx), C.c_float(ty),
                                       C.c_float(omega), int(scale_freeze), C.c_float(pos_cov), C.c_float(theta_cov),
                                       _ptr(z4), seed, step, index_base, self.stream()))

    def update_weights(self, raw_w, last_dist, n, w_out, info):
        check(self.lib.tdr_k_update_weights(_ptr(raw_w), _ptr(last_dist), n, _ptr(w_out), _ptr(info), self.stream()))

    def prefix_workspace(self, n):
        need = int(self.lib.tdr_prefix_workspace_bytes(n))
        if self._pws is None or self._pws.numel() < need:
            self._pws = self.empty((need,), torch.uint8)
        return self._pws

    def prefix(self, w, n, runmax):
        check(self.lib.tdr_k_prefix(_ptr(w), n, _ptr(runmax), _ptr(self.prefix_workspace(n)), self.stream()))

    def resample(self, runmax, n, n_new, shift, i_begin, i_end, idx):
        check(self.lib.tdr_k_resample(_ptr(runmax), n, n_new, C.c_float(shift), i_begin, i_end, _ptr(idx),
                                      self.stream()))

    def gather_states(self, src, idx, n_new, dst, src_shard=0):
        src_cap = src.shape[1] if src.dim() == 2 else 0
        check(self.lib.tdr_k_gather_states(_ptr(src), src_cap, src_shard, _ptr(idx), n_new, _ptr(dst), dst.shape[1],
                                           self.stream()))

    def save_ml_state(self, info, st, n, out12, src_shard=0):
        """out12[:7] = the SoA fields of particle argmax (info[0]), out12[8:12] its mlState; st: the [7][cap] planes, or
        with src_shard > 0 the all-gathered [rank][7][src_shard] buffer (particle_filter.cpp:145-147)."""
        cap = st.shape[1] if (st.dim() == 2 and src_shard == 0) else 0
        check(self.lib.tdr_k_save_ml_state(_ptr(info), _ptr(st), cap, src_shard, n, _ptr(out12), self.stream()))

    def resample_gather(self, runmax, n, n_new, shift, i_begin, i_end, idx, src, dst, info, out12, src_shard=0):
        """resample (shift: a float, or the device word holding the draw), gather_states and save_ml_state in one launch:
        idx, dst and out12 as those three leave them; src is the set BEFORE the resample, in either layout."""
        on_dev = hasattr(shift, "data_ptr")   # a tensor, or the DevPtr a generator pipe hands out
        src_cap = src.shape[1] if (src.dim() == 2 and src_shard == 0) else 0
        check(self.lib.tdr_k_resample_gather(_ptr(runmax), n, n_new, _ptr(shift) if on_dev else None,
                                             C.c_float(0.0 if on_dev else shift), i_begin, i_end, _ptr(idx), _ptr(src),
                                             src_cap, src_shard, _ptr(dst), dst.shape[1], _ptr(info), _ptr(out12),
                                             self.stream()))

    def mean_cov(self, st, n, about=None):
        """about: optional device tensor of 4 floats (computeCov about that mlState); None = about the mean."""
        out = self.empty((4800,))   # TDR_MEAN_COV_FLOATS: 24 results + reduction scratch
        check(self.lib.tdr_k_mean_cov(_ptr(st), st.shape[1], n, _ptr(about), _ptr(out), self.stream()))
        return out

    def sample_ml_states(self, st, n, num):
        """(num, 3) device tensor: mlState().head<3>() of particle min(n-1, i*n/num) (particle_filter.cpp:262-266)."""
        out = self.empty((num, 3))
        check(self.lib.tdr_k_sample_ml_states(_ptr(st), st.shape[1], n, num, _ptr(out), self.stream()))
        return out

    def gmm_select(self, samples, num_particles, num_gaussians, max_k=32):
        """Host: the deterministic mixture fit + cluster-count search of tdr_gmm.cpp.  samples: (m, 4) float64.
        Returns (k, means (k, 3) float32, covs (k, 3, 3) float32)."""
        x = np.ascontiguousarray(samples, np.float64)
        k = C.c_int(int(num_gaussians))
        means = np.zeros((max_k, 3), np.float32)
        covs = np.zeros((max_k, 9), np.float32)
        check(self.lib.tdr_gmm_select_host(x.ctypes.data_as(C.c_void_p), len(x), int(num_particles), C.byref(k), max_k,
                                           means.ctypes.data_as(C.c_void_p), covs.ctypes.data_as(C.c_void_p)))
        return k.value, means[: k.value].copy(), covs[: k.value].reshape(-1, 3, 3).copy()

    # ---- the mixture fit on the device (csrc/tdr_gmm.hip) -------------------------------------------------------
    def gmm_samples(self, ml3, num):
        """(num, 3) float {x, y, theta} -> (num, 4) double {x, y, 50 cos theta, 50 sin theta}, the host conversion's bits."""
        out = self.empty((num, 4), torch.float64)
        check(self.lib.tdr_k_gmm_samples(_ptr(ml3), num, _ptr(out), self.stream()))
        return out

    def gmm_fit(self, samples, k, max_iter=100):
        """The device twin of tdr_gmm_fit_host.  samples: (m, 4) float64 device tensor.
        Returns (w (k,), mu (k, 4), cov (k, 4, 4), ll, E-steps made) as NumPy / Python values."""
        m = samples.shape[0]
        out = self.zeros((int(self.lib.tdr_gmm_out_doubles(k)),), torch.float64)
        ws = self.empty((max(1, int(self.lib.tdr_gmm_workspace_bytes(m, k)) // 8),), torch.float64)
        check(self.lib.tdr_k_gmm_fit(_ptr(samples), m, k, max_iter, _ptr(out), _ptr(ws), self.stream()))
        o = out.cpu().numpy()
        return o[:k].copy(), o[k:5 * k].reshape(k, 4).copy(), o[5 * k:21 * k].reshape(k, 4, 4).copy(), float(o[21 * k]), \
            int(o[21 * k + 1])

    def gmm_candidates(self, num_gaussians, num_particles, m, max_k=_lib.GMM_MAX_K):
        """[k, k + 1 or 0, k - 1 or 0]: the fits tdr_gmm_select_host makes before it decides."""
        cand = (C.c_int * 3)()
        check(self.lib.tdr_gmm_candidates_host(int(num_gaussians), int(num_particles), int(m), int(max_k), cand))
        return list(cand)

    def gmm_select_device(self, ml3, num, num_particles, num_gaussians):
        """tdr_filter_compute_gmm_device's launches on torch buffers: ml3 (num, 3) float device tensor of the samples.
        Returns (k, means (k, 3) float32, covs (k, 3, 3) float32) like gmm_select."""
        import math
        x = self.gmm_samples(ml3, num)
        cand = self.gmm_candidates(num_gaussians, num_particles, num)
        jobs, pick, keep = [], _lib.GmmPickJobC(), []
        pick.k = cand[0]
        for j, kc in enumerate(cand):
            if not kc:
                continue
            out = self.zeros((21 * kc + 2,), torch.float64)
            ws = self.empty((num * kc,), torch.float64)
            keep += [out, ws]
            jobs.append(_lib.GmmJobC(x.data_ptr(), num, kc, 100, 0, out.data_ptr(), ws.data_ptr()))
            pick.cand[j] = out.data_ptr()
        rec = self.zeros((_lib.GMM_RECORD_DOUBLES,), torch.float64)
        pick.record = rec.data_ptr()
        jobs_c = (_lib.GmmJobC * len(jobs))(*jobs)
        jobs_d = self.to_device(np.frombuffer(bytes(jobs_c), np.uint8))
        pick_d = self.to_device(np.frombuffer(bytes(pick), np.uint8))
        check(self.lib.tdr_k_gmm_fit_jobs(_ptr(jobs_d), len(jobs), self.stream()))
        check(self.lib.tdr_k_gmm_pick(_ptr(pick_d), 1, self.stream()))
        r = rec.cpu().numpy()   # (the one read-back; it waits for the stream)
        k = int(r[0])
        if not 1 <= k <= _lib.GMM_MAX_K:
            raise _lib.TdrError("gmm_select_device: the device fit left no mixture")
        o = r[2:2 + 8 * k].reshape(k, 8)
        means = np.zeros((k, 3), np.float32)
        covs = np.zeros((k, 3, 3), np.float32)
        means[:, 0], means[:, 1] = o[:, 0], o[:, 1]
        means[:, 2] = [math.atan2(a, b) for a, b in zip(o[:, 3], o[:, 2])]   # (the host libm's, as tdr_gmm_select_host)
        covs[:, :2, :2] = o[:, 4:8].reshape(k, 2, 2)
        covs[:, 2, 2] = 1
        return k, means, covs

    # ---- KLD-sampling count (csrc/tdr_kld.hip; include/tdr.h, "KLD-sampling count") ---------------------------------
    def kld_keys(self, st, n, params):
        """The pose-bin keys of particles [0, n) of st (7, cap): NumPy uint64 (n,), KLD_NO_KEY where there is none."""
        out = self.empty((max(1, n),), torch.int64)
        check(self.lib.tdr_k_kld_keys(_ptr(st), st.shape[1], n, C.byref(params), _ptr(out), self.stream()))
        return out[:n].cpu().numpy().view(np.uint64).copy()

    def kld_workspace(self, n):
        """A key table for up to n particles (int64 device tensor; kld_count clears it)."""
        return self.empty((int(self.lib.tdr_kld_workspace_bytes(n)) // 8,), torch.int64)

    def kld_count(self, st, n, params, workspace=None):
        """(k, skipped): the distinct keys among particles [0, n) and the particles without a key.  One read-back."""
        if workspace is None:
            workspace = self.kld_workspace(n)
        if workspace.numel() * 8 < int(self.lib.tdr_kld_workspace_bytes(n)):
            raise ValueError("kld_count: the workspace is smaller than tdr_kld_workspace_bytes(n)")
        out = self.empty((2,), torch.int64)
        check(self.lib.tdr_k_kld_count(_ptr(st), st.shape[1], n, C.byref(params), _ptr(workspace), _ptr(out), self.stream()))
        k, skipped = out.cpu().tolist()
        return int(k), int(skipped)

    def kld_count_jobs(self, sts, ns, params):
        """kld_count of several state tensors in one launch (the job table of tdr_k_kld_count_jobs): [(k, skipped)]."""
        slots = [int(self.lib.tdr_kld_workspace_bytes(n)) // 8 if n >= 1 else 0 for n in ns]
        tables = self.empty((max(1, sum(slots)),), torch.int64)
        tables.fill_(-1)
        out = self.zeros((len(sts), 2), torch.int64)
        jobs, at = [], 0
        for i, (st, n) in enumerate(zip(sts, ns)):
            jobs.append(_lib.KldJobC(st.data_ptr(), st.shape[1], n, tables.data_ptr() + 8 * at, slots[i],
                                     out.data_ptr() + 16 * i))
            at += slots[i]
        jobs_d = self.to_device(np.frombuffer(bytes((_lib.KldJobC * len(jobs))(*jobs)), np.uint8).copy())
        check(self.lib.tdr_k_kld_count_jobs(_ptr(jobs_d), len(jobs), C.byref(params), self.stream()))
        return [(int(a), int(b)) for a, b in out.cpu().tolist()]

    def kld_target(self, k, params, last_count, max_count):
        """The next update's count from k occupied bins (tdr_kld_bound_host, tdr_kld_target_host)."""
        n_kld = self.lib.tdr_kld_bound_host(int(k), C.c_double(params.epsilon), C.c_double(params.z))
        return int(self.lib.tdr_kld_target_host(n_kld, int(last_count), int(params.n_min), int(max_count)))

    # ---- recovery injection (csrc/tdr_recover.hip; include/tdr.h, "recovery injection") ------------------------------
    def road_cells(self, dmap):
        """The road list of a DeviceMap: the cell indices r * cols + c, ascending, of the cells whose class-1 slot is below
        1 (int32 device tensor holding uint32 words).  One read-back (the length)."""
        cells = self.empty((dmap.rows * dmap.cols,), torch.int32)
        ws = self.empty((max(1, int(self.lib.tdr_map_road_workspace_bytes(dmap.rows, dmap.cols))),), torch.uint8)
        count = self.zeros((1,), torch.int64)
        check(self.lib.tdr_k_map_road_cells(C.byref(dmap.desc), _ptr(cells), _ptr(count), _ptr(ws), self.stream()))
        return cells[: int(count.item())]

    def inject(self, st, n, dmap, road, seed, draw, threshold24, heading_mode, slot_begin=0, count=True):
        """tdr_k_inject on slots [0, n) of st (7, cap): every slot whose Philox word falls below threshold24 becomes a fresh
        particle on a cell of `road` (road_cells).  Returns the number of injected slots (one read-back), or None with
        count=False (no read-back, no wait)."""
        out = self.zeros((1,), torch.int64) if count else None
        check(self.lib.tdr_k_inject(_ptr(st), st.shape[1], n, slot_begin, C.byref(dmap.desc), _ptr(road), road.numel(),
                                    int(seed), int(draw), int(threshold24), int(heading_mode), _ptr(out), self.stream()))
        return int(out.item()) if count else None

    def inject_jobs(self, sts, ns, dmaps, roads, seeds, draws, thresholds, heading_mode, slot_begins=None):
        """inject of several state tensors in one launch (the job table of tdr_k_inject_jobs): the injected counts."""
        out = self.zeros((len(sts),), torch.int64)
        jobs = []
        for i, (st, n, dm, road) in enumerate(zip(sts, ns, dmaps, roads)):
            jobs.append(_lib.InjectJobC(st.data_ptr(), st.shape[1], n, 0 if slot_begins is None else slot_begins[i],
                                        road.data_ptr(), road.numel(), dm.cols, dm.resolution, int(seeds[i]), int(draws[i]),
                                        int(thresholds[i]), int(heading_mode), out.data_ptr() + 8 * i))
        jobs_d = self.to_device(np.frombuffer(bytes((_lib.InjectJobC * len(jobs))(*jobs)), np.uint8).copy())
        check(self.lib.tdr_k_inject_jobs(_ptr(jobs_d), len(jobs), self.stream()))
        return [int(v) for v in out.cpu().tolist()]

    def inject_threshold(self, p):
        """tdr_inject_threshold_host: floor(p * 2^24), clamped to [0, 2^24]."""
        return int(self.lib.tdr_inject_threshold_host(C.c_double(p)))

    # ---- sensor resetting (csrc/tdr_recover_sensor.hip; include/tdr.h, "sensor resetting") -----------------------------
    def inject_list(self, n, seed, draw, threshold24, slot_begin=0, max_blocks=0):
        """tdr_k_inject_list: the ascending local indices of the slots of [0, n) that inject would write (int32 device
        tensor).  One read-back (the length)."""
        lst = self.empty((max(n, 1),), torch.int32)
        ws = self.empty((max(8, int(self.lib.tdr_inject_list_workspace_bytes(n))),), torch.uint8)
        count = self.zeros((1,), torch.int64)
        check(self.lib.tdr_k_inject_list(n, slot_begin, int(seed), int(draw), int(threshold24), _ptr(lst), _ptr(count), _ptr(ws),
                                         int(max_blocks), self.stream()))
        return lst[: int(count.item())]

    def inject_candidates(self, st, n, lst, first, m, candidates, dmap, road, seed, draw, heading_mode, cand_st, slot_begin=0):
        """tdr_k_inject_candidates: the states of the `candidates` candidates of list entries [first, first + m) into
        cand_st (7, cand_cap), candidate (e - first) * candidates + j."""
        check(self.lib.tdr_k_inject_candidates(_ptr(st), st.shape[1], n, slot_begin, _ptr(lst), first, m, int(candidates),
                                               C.byref(dmap.desc), _ptr(road), road.numel(), int(seed), int(draw), int(heading_mode),
                                               _ptr(cand_st), cand_st.shape[1], self.stream()))

    def inject_select(self, st, n, lst, first, m, candidates, cand_st, cand_w, pick=None, written=None):
        """tdr_k_inject_select: every slot of list entries [first, first + m) takes the first of its candidates of the
        largest weight (a NaN counts as -1); pick (int32, m) and written (int64, 1; incremented) are optional."""
        check(self.lib.tdr_k_inject_select(_ptr(st), st.shape[1], n, _ptr(lst), first, m, int(candidates), _ptr(cand_st),
                                           cand_st.shape[1], _ptr(cand_w), _ptr(pick), _ptr(written), self.stream()))

    # ---- pose-grid search (csrc/tdr_grid.hip; include/tdr.h, "pose-grid search") -----------------------------------------
    def grid_list(self, dmap, spec, max_blocks=0):
        """tdr_k_grid_list: the ascending lattice points of spec (a _lib.GridSpecC) that stand on a cell (with road_only: a
        road cell) of the DeviceMap (int32 device tensor).  One read-back (the length)."""
        G = int(spec.nx) * int(spec.ny)
        lst = self.empty((max(G, 1),), torch.int32)
        ws = self.empty((max(8, int(self.lib.tdr_grid_list_workspace_bytes(int(spec.nx), int(spec.ny)))),), torch.uint8)
        count = self.zeros((1,), torch.int64)
        check(self.lib.tdr_k_grid_list(C.byref(dmap.desc), C.byref(spec), _ptr(lst), _ptr(count), _ptr(ws), int(max_blocks),
                                       self.stream()))
        return lst[: int(count.item())]

    def grid_candidates(self, dmap, spec, lst, first, m, cand_st):
        """tdr_k_grid_candidates: the states of the H candidates of list entries [first, first + m) into cand_st
        (7, cand_cap), candidate (e - first) * H + h."""
        check(self.lib.tdr_k_grid_candidates(C.byref(dmap.desc), C.byref(spec), _ptr(lst), lst.numel(), first, m, _ptr(cand_st),
                                             cand_st.shape[1], self.stream()))

    def grid_planes(self, spec, vol=False):
        """The W and T planes (and the H-deep vol) of a lattice, filled with the NaN of unlisted points."""
        G = int(spec.nx) * int(spec.ny)
        nan = lambda n: self.to_device(np.full(n, 0x7FC00000, np.uint32).view(np.float32))
        return nan(G), nan(G), (nan(G * int(spec.n_headings)) if vol else None)

    def grid_reduce(self, spec, lst, first, m, cand_st, cand_w, w_plane, t_plane, vol=None):
        """tdr_k_grid_reduce: W, T and the vol column of list entries [first, first + m) from their H weights and the states
        as scoring left them."""
        check(self.lib.tdr_k_grid_reduce(C.byref(spec), _ptr(lst), lst.numel(), first, m, _ptr(cand_st), cand_st.shape[1],
                                         _ptr(cand_w), _ptr(w_plane), _ptr(t_plane), _ptr(vol), self.stream()))

    def grid_peaks(self, dmap, spec, w_plane, t_plane, radius, max_peaks):
        """tdr_k_grid_peaks: (the first min(max_peaks, n_peaks) peaks as a _lib.GRID_PEAK_DTYPE array, n_peaks).  One
        read-back."""
        ws = self.empty((max(8, int(self.lib.tdr_grid_peaks_workspace_bytes(int(spec.nx), int(spec.ny)))),), torch.uint8)
        count = self.zeros((1,), torch.int64)
        peaks = self.zeros((max(int(max_peaks), 1), 4), torch.int32)
        check(self.lib.tdr_k_grid_peaks(C.byref(dmap.desc), C.byref(spec), _ptr(w_plane), _ptr(t_plane), int(radius), int(max_peaks),
                                        _ptr(peaks), _ptr(count), _ptr(ws), self.stream()))
        n = int(count.item())
        out = peaks.cpu().numpy().view(_lib.GRID_PEAK_DTYPE).reshape(-1)
        return out[: min(int(max_peaks), n)].copy(), n

    # ---- the particle picture (csrc/tdr_viz.hip) ---------------------------------------------------------------
    def viz_planes(self, H, W):
        """The four bit planes of an H x W picture, as one int32 tensor (cleared by viz_draw)."""
        words = int(self.lib.tdr_viz_plane_words(H, W))
        if words == 0:
            raise _lib.TdrError(f"no picture of {H} x {W} pixels")
        return self.zeros((4 * words,), torch.int32)

    def viz_draw(self, st, n, background, planes, segs, out_h, out_w, out=None):
        """background: (H, W, 3) uint8 device tensor; segs: (m, 5) int32 overlay segments (host array).  Clears the
        planes, draws particles and overlay and composes the published (out_h, out_w, 3) uint8 device tensor."""
        H, W = int(background.shape[0]), int(background.shape[1])
        if out is None:
            out = self.empty((out_h, out_w, 3), torch.uint8)
        planes.zero_()
        check(self.lib.tdr_k_viz_particles(_ptr(st), st.shape[1], n, H, W, _ptr(planes), self.stream()))
        if len(segs):
            segs_d = self.to_device(np.ascontiguousarray(segs, np.int32))
            check(self.lib.tdr_k_viz_segments(_ptr(segs_d), len(segs), H, W, _ptr(planes), self.stream()))
        check(self.lib.tdr_k_viz_compose(_ptr(background), H, W, _ptr(planes), out_h, out_w, _ptr(out), self.stream()))
        return out

    # ---- the fleet picture (include/tdr.h, "the fleet picture") ------------------------------------------------------
    def viz_compose_fleet(self, jobs, k, palette, background, green_plane, out_h, out_w, out=None):
        """tdr_k_viz_compose_fleet: jobs is a device uint8 tensor holding k tdr_viz_job records (their planes 0 - 2
        drawn), palette (k, 3, 3) uint8 on the host, background (H, W, 3) uint8 and green_plane int32 device tensors.
        Returns the published (out_h, out_w, 3) uint8 device tensor."""
        H, W = int(background.shape[0]), int(background.shape[1])
        pal = np.ascontiguousarray(palette, np.uint8)
        if pal.size != 9 * k:
            raise ValueError("viz_compose_fleet: the palette is (k, 3, 3) BGR bytes")
        if out is None:
            out = self.empty((out_h, out_w, 3), torch.uint8)
        check(self.lib.tdr_k_viz_compose_fleet(_ptr(jobs), int(k), pal.ctypes.data_as(C.c_void_p), _ptr(background), H, W,
                                               _ptr(green_plane), int(out_h), int(out_w), _ptr(out), self.stream()))
        return out

    def viz_draw_fleet(self, robots, background, palette, arrows, out_h, out_w):
        """The fleet picture's three launches on torch buffers.  robots: per robot (st, n, segs, best) — st a (7, cap)
        float device tensor, segs its estimate as (m, 5) int32 host segments (viz_overlay_host with best = None and no
        arrows), best a device float tensor {x, y, theta} or None; arrows: the caller's (m, 4) list or None."""
        H, W = int(background.shape[0]), int(background.shape[1])
        k = len(robots)
        words = int(self.lib.tdr_viz_plane_words(H, W))
        planes = self.zeros(((3 * k + 1) * words,), torch.int32)   # robot i's three at 3 i, the green plane last
        green = viz_overlay_host(np.zeros((0, 3)), np.zeros((0, 9)), None, arrows, H)
        jobs, keep, max_n, max_segs = (_lib.VizJobC * k)(), [], 0, 0
        for i, (st, n, segs, best) in enumerate(robots):
            segs = np.ascontiguousarray(segs, np.int32).reshape(-1, 5)
            if i == k - 1:   # (its plane 3 is the green plane)
                segs = np.concatenate([segs, green])
            segs_d = self.to_device(segs if len(segs) else np.zeros((1, 5), np.int32))
            keep.append(segs_d)
            j = jobs[i]
            j.st, j.cap, j.n, j.H, j.W = st.data_ptr(), st.shape[1], int(n), H, W
            j.planes = planes.data_ptr() + 4 * 3 * i * words
            j.background, j.segs, j.n_segs = background.data_ptr(), segs_d.data_ptr(), len(segs)
            j.best = best.data_ptr() if best is not None else None
            max_n, max_segs = max(max_n, int(n)), max(max_segs, len(segs))
        jobs_d = self.to_device(np.frombuffer(jobs, np.uint8))
        check(self.lib.tdr_k_viz_particles_jobs(_ptr(jobs_d), k, max_n, self.stream()))
        check(self.lib.tdr_k_viz_segments_jobs(_ptr(jobs_d), k, max_segs, self.stream()))
        return self.viz_compose_fleet(jobs_d, k, palette, background, planes[3 * k * words:], out_h, out_w)

    # ---- the scan picture (csrc/tdr_scan_viz.hip) ----------------------------------------------------------------
    @staticmethod
    def _colour_table(lut_bgr):
        lut = np.ascontiguousarray(lut_bgr, np.uint8)
        if lut.size != 768:
            raise ValueError("the colour table is 256 BGR triplets")
        return lut

    def scan_picture(self, imgs, ncls, rows, cols, unflatten, lut_bgr, out=None):
        """imgs: device float32 [ncls][rows*cols] (the render layout) -> the (cols, rows, 3) uint8 device picture."""
        unf = np.ascontiguousarray(unflatten, np.int32)
        if unf.size < ncls:
            raise ValueError(f"unflatten has {unf.size} entries, the render {ncls} classes")
        lut = self._colour_table(lut_bgr)
        if out is None:
            out = self.empty((cols, rows, 3), torch.uint8)
        check(self.lib.tdr_k_scan_picture(_ptr(imgs), int(ncls), int(rows) * int(cols), unf.ctypes.data_as(C.c_void_p),
                                          lut.ctypes.data_as(C.c_void_p), _ptr(out), self.stream()))
        return out

    def analog_picture(self, img, rows, cols, scale, out=None):
        """img: one device float32 layer [rows*cols] -> the (cols, rows, 3) grey device picture."""
        if out is None:
            out = self.empty((cols, rows, 3), torch.uint8)
        check(self.lib.tdr_k_analog_picture(_ptr(img), int(rows) * int(cols), C.c_float(scale), _ptr(out), self.stream()))
        return out

    def label_picture(self, labels, lut_bgr, out=None):
        """labels: (H, W) uint8 device tensor -> the (H, W, 3) uint8 device picture lut_bgr[labels]."""
        lut = self._colour_table(lut_bgr)
        H, W = int(labels.shape[0]), int(labels.shape[1])
        if out is None:
            out = self.empty((H, W, 3), torch.uint8)
        check(self.lib.tdr_k_label_picture(_ptr(labels), H * W, lut.ctypes.data_as(C.c_void_p), _ptr(out), self.stream()))
        return out

    def set_scale(self, st, n, scale_dev):
        check(self.lib.tdr_k_set_scale(_ptr(st), st.shape[1], n, _ptr(scale_dev), self.stream()))

    def shift_init(self, st, n, dx, dy):
        check(self.lib.tdr_k_shift_init(_ptr(st), st.shape[1], n, C.c_float(dx), C.c_float(dy), self.stream()))

    def locality_order(self, st, n, rows, cols, perm):
        need = int(self.lib.tdr_locality_tmp_ints(n, rows, cols))
        tmp = self.empty((need,), torch.int32)
        check(self.lib.tdr_k_locality_order(_ptr(st), st.shape[1], n, rows, cols, _ptr(perm), _ptr(tmp),
                                            self.stream()))

    def locality_order_pose(self, st, n, rows, cols, perm, theta_radius):
        """Order for windows that rotate with the particle (Cartesian scoring): Morton code of (x, y, theta)."""
        need = int(self.lib.tdr_locality_pose_tmp_ints(n))
        tmp = self.empty((need + 2,), torch.int32)
        check(self.lib.tdr_k_locality_order_pose(_ptr(st), st.shape[1], n, rows, cols, C.c_float(theta_radius),
                                                 _ptr(perm), _ptr(tmp), self.stream()))

    def states_to_device(self, states_aos, st, n):
        """states_aos: numpy structured array with the reference's 28-byte State layout."""
        raw = self.to_device(np.ascontiguousarray(states_aos).view(np.uint8).reshape(-1))
        check(self.lib.tdr_k_states_aos_to_soa(_ptr(raw), n, _ptr(st), st.shape[1], self.stream()))
        self.synchronize()

    def states_to_host(self, st, n, dtype):
        raw = self.empty((n * 28,), torch.uint8)
        check(self.lib.tdr_k_states_soa_to_aos(_ptr(st), st.shape[1], n, _ptr(raw), self.stream()))
        return raw.cpu().numpy().view(dtype).reshape(-1).copy()

    def su_order(self, st, n, nb, span, perm=None, workspace=None):
        """tdr_k_su_order (include/tdr.h): the ordering passes of an integer-form launch alone.  Returns int32 tensors
        (slots, keys, counts) and whether the bucket sort ran; `workspace`: an int32 tensor of at least
        tdr_k_su_order_workspace_ints(n, nb) words."""
        need = int(self.lib.tdr_k_su_order_workspace_ints(n, nb))
        if workspace is None:
            workspace = self.empty((need,), torch.int32)
        if workspace.numel() < need:
            raise ValueError(f"su_order: workspace of {workspace.numel()} words, {need} needed")
        slots = self.empty((int(self.lib.tdr_k_su_order_slots(n, nb)),), torch.int32)
        keys = self.empty((n,), torch.int32)
        counts = self.empty((3,), torch.int32)
        bucket = C.c_int(-1)
        check(self.lib.tdr_k_su_order(_ptr(st), st.shape[1], n, _ptr(perm) if perm is not None else None, nb,
                                      C.c_float(span), _ptr(workspace), _ptr(slots), _ptr(keys), _ptr(counts), C.byref(bucket),
                                      self.stream()))
        return slots, keys, counts, bool(bucket.value)

    def score_prep(self, m, scan_pk, res, st, n, perm=None, uniform_scale=0.0, n_total=0, ctx=None, span=0.0, workspace=None):
        """tdr_k_score_prep (include/tdr.h): the ordering passes and the scan-side preparation of an integer-form scoring call
        alone.  Returns (layout, products): the 16 layout words and a dict of tensors — utab, tab_su, desc, bbox, tab_ray,
        desc_ray (int16 view), rad_ray, list, tail.  `workspace`: a float tensor of tdr_score_workspace_floats floats."""
        if ctx is not None:
            check(self.lib.tdr_score_ctx_set_polar_factors(ctx.handle, _ptr(getattr(m, "fac", None)), m.nb, m.nr))
        h = ctx.handle if ctx is not None else C.c_void_p(0)
        lay = (C.c_int64 * 16)()
        head = (C.byref(m.desc), _ptr(m.tab), _ptr(scan_pk), m.nb, m.nr, C.c_float(res), _ptr(st), st.shape[1], n, n_total,
                _ptr(perm), C.c_float(uniform_scale), C.c_float(span))
        check(self.lib.tdr_k_score_prep(*head, None, h, lay, None, self.stream()))
        group, nchunks, _, _, _, _, _, T, nbins, nsect, tail = [int(v) for v in lay[:11]]
        ws = workspace if workspace is not None else self._workspace(m.ncls, m.nb, m.nr, n, n_total)
        prod = {"utab": self.zeros((m.nr * m.nb, 2)), "tab_su": self.zeros((nbins, 2)),
                "desc": self.zeros((nbins, 4), torch.int32), "bbox": self.zeros((nchunks, nsect, 4)),
                "tab_ray": self.zeros((T, 2)), "desc_ray": self.zeros(((T + 1) // 2,), torch.int32),
                "rad_ray": self.zeros((T // m.nb,)), "list": self.zeros((m.nb * m.nr,), torch.int32),
                "tail": self.zeros((tail,), torch.int32)}
        out = (C.c_void_p * 9)(*[_ptr(prod[k]) for k in ("utab", "tab_su", "desc", "bbox", "tab_ray", "desc_ray", "rad_ray",
                                                           "list", "tail")])
        check(self.lib.tdr_k_score_prep(*head, _ptr(ws), h, lay, out, self.stream()))
        prod["desc_ray"] = prod["desc_ray"].view(torch.int16)
        return [int(v) for v in lay], prod

    def tuning(self, name, value=-1):
        """tdr_config_tuning (include/tdr.h): value < 0 queries; returns the value in force, -1 for an unknown name."""
        return int(self.lib.tdr_config_tuning(name.encode(), value))

    # ---- host RNG (the reference's shared std::mt19937) -------------------------------------------------------
    def rng_create(self, seed):
        return C.c_void_p(self.lib.tdr_rng_create(C.c_uint32(seed & 0xFFFFFFFF)))

    # the same generator continued on the device (csrc/tdr_rng.hip): state = 640 uint32 words (include/tdr.h)
    device_rng = True
    fused_resample = True   # resample_gather: the unsharded update's tail in one launch (tdr_k_resample_gather)

    def rng_state_to_device(self, rng):
        words = np.zeros(640, np.uint32)
        check(self.lib.tdr_rng_get_state_host(rng, words.ctypes.data_as(C.c_void_p)))
        return self.to_device(words.view(np.int32))

    def rng_state_to_host(self, rng, state_dev):
        words = np.ascontiguousarray(state_dev.cpu().numpy()).view(np.uint32)
        check(self.lib.tdr_rng_set_state_host(rng, words.ctypes.data_as(C.c_void_p)))

    def rng_propagate_normals_dev(self, state_dev, n, lo, hi, scale_freeze, z4_out, n_max):
        need = int(self.lib.tdr_rng_dev_workspace_bytes(max(n, n_max)))
        if getattr(self, "_rws", None) is None or self._rws.numel() < need:
            self._rws = self.empty((need,), torch.uint8)
        check(self.lib.tdr_k_rng_propagate_normals(_ptr(state_dev), n, lo, hi, int(scale_freeze), _ptr(z4_out),
                                                   _ptr(self._rws), self.stream()))

    def rng_uniform_dev(self, state_dev, out_dev):
        check(self.lib.tdr_k_rng_uniform(_ptr(state_dev), _ptr(out_dev), self.stream()))

    def resample_dev(self, runmax, n, n_new, shift_dev, i_begin, i_end, idx):
        check(self.lib.tdr_k_resample_dev(_ptr(runmax), n, n_new, _ptr(shift_dev), i_begin, i_end, _ptr(idx), self.stream()))

    def rng_pipe_create(self, n_max):
        """A tdr_rng_pipe (include/tdr.h): one filter's generator on the device, drawing ahead of the step."""
        h = C.c_void_p(0)
        check(self.lib.tdr_rng_pipe_create(n_max, C.byref(h)))
        return RngPipe(self, h)

    def rng_uniform(self, rng):
        return float(self.lib.tdr_rng_uniform_host(rng))

    def init_particles(self, rng, maps_cm_host, ncls, rows, cols, resolution, fp, max_num, dtype):
        out = np.zeros(max_num + 16, dtype)
        n = C.c_int64(0)
        check(self.lib.tdr_init_particles_host(rng, maps_cm_host.ctypes.data_as(C.c_void_p), ncls, rows, cols,
                                               C.c_float(resolution), C.byref(fp), max_num,
                                               out.ctypes.data_as(C.c_void_p), C.byref(n)))
        return out[: min(n.value, max_num + 16)].copy()

    def init_particles_count(self, fp, max_num):
        """Particles initializeParticles' loop keeps (tdr_init_particles_count)."""
        return int(self.lib.tdr_init_particles_count(C.byref(fp), max_num))

    def init_particles_dev(self, state_dev, dmap, fp, max_num, lo, hi, st):
        """The same loop on a device generator state (tdr_k_init_particles): particles [lo, hi) into st; returns the
        count the loop keeps."""
        n = C.c_int64(0)
        ws = self.empty((int(self.lib.tdr_init_workspace_bytes()),), torch.uint8)
        check(self.lib.tdr_k_init_particles(_ptr(state_dev), C.byref(dmap.desc), C.byref(fp), max_num, lo, hi, _ptr(st),
                                            st.shape[1], C.byref(n), _ptr(ws), self.stream()))
        return n.value

    def propagate_normals(self, rng, n, scale_freeze):
        z = np.empty((n, 4), np.float32)
        check(self.lib.tdr_propagate_normals_host(rng, n, int(scale_freeze), z.ctypes.data_as(C.c_void_p)))
        return z
