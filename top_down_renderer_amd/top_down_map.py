"""TopDownMap / TopDownMapPolar — host-side mirrors of the reference classes (include/top_down_render/top_down_map.h:52-102,
top_down_map_polar.h:6-22) holding the map on the device for the HIP kernels.

Map content is taken in the form the reference's load-time code produces (src/top_down_map.cpp:289-326): per-class
truncated distance maps + unknown mask, or built on the GPU from a label image, a raster cache, an SVG vector map
(loadVectorMap; parse_svg returns the polygons the reference's loadSvg keeps) or a colour raster map (loadColorRasterMap;
png_read_color returns the BGR image cv::imread gives, color_index is color2Ind on the GPU).
"""
from dataclasses import dataclass, field

import numpy as np
import torch


def parse_svg(path):
    """The polygons TopDownMap::loadSvg (src/top_down_map.cpp:66-110) keeps of an SVG file (host only, no GPU):
    (size, polygons) with size = (width, height) as floats and polygons a list of (fill_key, (n, 2) float32 vertices
    (x, height - y)).  fill_key = the shape's 0xBBGGRR fill colour (0 for fill="none" / no fill), None for a gradient."""
    from . import _lib
    from .kernels import svg_parse
    size, keys, offs, verts = svg_parse(path)
    polys = [(None if int(k) == _lib.TDR_SVG_NO_KEY else int(k), verts[offs[p]:offs[p + 1]].copy())
             for p, k in enumerate(keys)]
    return (float(size[0]), float(size[1])), polys


def svg_fill_key(rgb):
    """The key loadSvg compares a shape's fill with (:82-84) for an (r, g, b) colour: c[0] << 16 | c[1] << 8 | c[2]."""
    r, g, b = (int(x) & 0xFF for x in rgb[:3])
    return (r << 16) | (g << 8) | b


def color_key(bgr):
    """The key of a BGR pixel (cv::imread's channel order) as the colour map's lookup compares it: b << 16 | g << 8 | r,
    which is svg_fill_key of the same colour's unpackColor bytes — an SVG fill #ff0000 and a PNG pixel RGB (255, 0, 0)
    have the same key 0x0000ff.  bgr: one (b, g, r) triple -> int, or an (..., 3) array -> uint32 array of keys."""
    a = np.asarray(bgr)
    if a.ndim == 1:
        b, g, r = (int(x) & 0xFF for x in a[:3])
        return (b << 16) | (g << 8) | r
    a = a.astype(np.uint32)
    return (a[..., 0] << 16) | (a[..., 1] << 8) | a[..., 2]


def png_read_color(path):
    """The BGR8 image cv::imread(path) gives for a PNG file (host only, no GPU): (H, W, 3) uint8, row 0 = top."""
    from .kernels import png_read_color as read
    return read(path)


def color_index(bgr, fill_keys, kernels=None):
    """SemanticColorLut::color2Ind on the GPU, taken as the exact inverse of ind2Color over the LUT: (H, W, 3) uint8
    BGR -> (H, W) uint8, the smallest LUT index i with color_key(pixel) == fill_keys[i], 255 where none matches."""
    if kernels is None:
        from .kernels import HipKernels
        kernels = HipKernels()
    return kernels.color_index(bgr, fill_keys)


@dataclass
class Params:
    """TopDownMap::Params (top_down_map.h:54-62), minus the load-time colour LUT."""
    map_path: str = ""
    flatten_lut: list = field(default_factory=list)
    num_classes: int = 0
    exclusive_classes: list = field(default_factory=list)
    resolution: float = 1.0
    out_of_bounds_const: float = 5.0   # read but unused by the reference: every OOB write is a literal 0


class TopDownMap:
    def __init__(self, params, class_maps=None, class_mask=None, kernels=None):
        """class_maps: (ncls, H, W) float32 indexed [cls, row(y), col(x)]; class_mask: (H, W) uint8, 1 = unknown."""
        if kernels is None:
            from .kernels import HipKernels
            kernels = HipKernels()   # raises without the built extension / a GPU: no CPU fallback
        self.k = kernels
        self.params_ = params
        self.map_center_ = (0, 0)
        self.have_map_ = False
        self.dev = None
        self.geo_constant_one_ = False   # True after updateMap(label image): the reference leaves geo_maps_ at 1 there
        if class_maps is not None:
            self._load(class_maps, class_mask)

    def _load(self, class_maps, class_mask):
        class_maps = np.ascontiguousarray(class_maps, np.float32)
        class_mask = np.ascontiguousarray(class_mask, np.uint8)
        ncls, H, W = class_maps.shape
        if self.params_.num_classes and self.params_.num_classes != ncls:
            raise ValueError("num_classes does not match the class maps")
        self.params_.num_classes = ncls
        self.rows, self.cols = H, W
        # host copy in the reference's column-major layout (class_maps_): needed by getClassesAtPoint / particle init
        self.maps_cm_host = np.ascontiguousarray(np.transpose(class_maps, (0, 2, 1)))
        self.dev = self.k.make_map(class_maps, class_mask, self.params_.resolution)
        self.have_map_ = True

    # top_down_map.cpp:146-157
    def updateMap(self, class_maps, class_mask=None, map_center=(0, 0)):
        """updateMap(label_img, map_center) like the reference (a cv::Mat of class ids), or
        updateMap(class_maps, class_mask, map_center) with distance maps computed elsewhere."""
        if class_mask is None or np.ndim(class_maps) == 2:
            if class_mask is not None and np.ndim(class_mask) == 1:
                map_center = class_mask
            return self.loadCompressedRasterMap(class_maps, map_center)
        self.map_center_ = (int(map_center[0]), int(map_center[1]))
        old = self.dev
        self.geo_constant_one_ = False
        self._load(class_maps, class_mask)
        if old is not None and getattr(old, "nb", 0):
            self.k.set_polar_table(self.dev, old.nb, old.nr, old.ang_res)

    # top_down_map.cpp:116-144 + 289-326, and updateMap :146-157 for a class-index image (cv::Mat CV_8UC1)
    def loadCompressedRasterMap(self, label_img, map_center=(0, 0)):
        """label_img: (H, W) uint8 image of raw class ids, row 0 = top like a cv::Mat; params_.flatten_lut maps raw id
        -> flattened class.  Class binary maps, the exact Euclidean distance transform, truncation at 50 and the
        unknown mask are all computed on the GPU."""
        p = self.params_
        if not p.num_classes or not len(p.flatten_lut):
            raise ValueError("Params.num_classes and Params.flatten_lut are needed to ingest a label image")
        old = self.dev
        self.geo_constant_one_ = True            # loadCompressedRasterMap :126-133, never recomputed by updateMap
        self.dev = self.k.make_map_from_labels(label_img, p.flatten_lut, p.num_classes, p.resolution)
        self.rows, self.cols = self.dev.rows, self.dev.cols
        maps_cm, _ = self.k.unpack_map(self.dev)
        self.maps_cm_host = maps_cm            # column-major host copy (class_maps_), for getClassesAtPoint / init
        self.map_center_ = (int(map_center[0]), int(map_center[1]))
        # `if (!class_maps_[1].isZero(0)) have_map_ = true` (:150): a map without any road is not usable
        if p.num_classes > 1 and bool((self.maps_cm_host[1] != 0).any()):
            self.have_map_ = True
        if old is not None and getattr(old, "nb", 0):
            self.k.set_polar_table(self.dev, old.nb, old.nr, old.ang_res)

    def updateMapIncremental(self, label_img, map_center=(0, 0)):
        """loadCompressedRasterMap's end state, reached by rebuilding only what changed since the last image
        (kernels.update_map_from_labels, csrc/tdr_map_incr.hip).  Returns the number of cells whose class changed, or -1
        when it took the full path: no label image kept from an earlier call, a different shape / LUT / class count /
        resolution, or a change over more than half the map."""
        p = self.params_
        if not p.num_classes or not len(p.flatten_lut):
            raise ValueError("Params.num_classes and Params.flatten_lut are needed to ingest a label image")
        label_img = np.ascontiguousarray(label_img, np.uint8)
        lut = np.ascontiguousarray(p.flatten_lut, np.int32).ravel()
        dev = self.dev
        ing = getattr(dev, "ingest", None)
        res = None
        if (ing is not None and ing.shape == label_img.shape and ing.ncls == p.num_classes
                and ing.resolution == float(p.resolution) and np.array_equal(ing.lut, lut)):
            res = self.k.update_map_from_labels(dev, label_img, max_cells=int(dev.rows * dev.cols * 0.5))
        if res is None:   # the full path, keeping what the next call needs
            old = self.dev
            self.geo_constant_one_ = True
            self.dev = self.k.make_map_from_labels(label_img, p.flatten_lut, p.num_classes, p.resolution,
                                                   keep_ingest=True)
            self.rows, self.cols = self.dev.rows, self.dev.cols
            maps_cm, _ = self.k.unpack_map(self.dev)
            self.maps_cm_host = maps_cm
            self.map_center_ = (int(map_center[0]), int(map_center[1]))
            if p.num_classes > 1 and bool((self.maps_cm_host[1] != 0).any()):
                self.have_map_ = True
            if old is not None and getattr(old, "nb", 0):
                self.k.set_polar_table(self.dev, old.nb, old.nr, old.ang_res)
            return -1
        changed, tiles = res
        if len(tiles):   # the host copy changes in the affected tiles only
            maps_t, _ = self.k.gather_tiles(dev, tiles)
            tx_n = (dev.cols + 31) // 32
            for b, t in enumerate(tiles):
                ty, tx = divmod(int(t), tx_n)
                r0, c0 = ty * 32, tx * 32
                nr, nc = min(32, dev.rows - r0), min(32, dev.cols - c0)
                self.maps_cm_host[:, c0:c0 + nc, r0:r0 + nr] = maps_t[b, :, :nc, :nr]
                if not self.have_map_ and p.num_classes > 1 and bool((maps_t[b, 1, :nc, :nr] != 0).any()):
                    self.have_map_ = True
        self.map_center_ = (int(map_center[0]), int(map_center[1]))
        return changed

    # top_down_map.cpp:197-224 — the raster cache: a directory of class<i>.png (8-bit grey, 0 inside the class, flipped)
    def saveRasterizedMaps(self, path):
        import os
        os.makedirs(path, exist_ok=True)
        maps_cm, mask_cm = self.k.unpack_map(self.dev)
        for c in range(self.dev.ncls):
            inside = (maps_cm[c].T == 0) & (mask_cm.T == 0)                  # [row][col], row 0 = bottom
            self.k.png_write_gray8(os.path.join(path, f"class{c}.png"), np.where(inside, 0, 255).astype(np.uint8)[::-1])

    def loadRasterizedMaps(self, map_path, map_center=(0, 0)):
        """The constructor's path for a raster-cache directory (:42-58): rasters -> distance maps on the GPU."""
        import os
        p = self.params_
        planes = np.stack([self.k.png_read_gray8(os.path.join(map_path, f"class{c}.png")) for c in range(p.num_classes)])
        old = self.dev
        self.geo_constant_one_ = False
        self.dev = self.k.make_map_from_rasters(planes, p.resolution)
        self.rows, self.cols = self.dev.rows, self.dev.cols
        maps_cm, _ = self.k.unpack_map(self.dev)
        self.maps_cm_host = maps_cm
        self.map_center_ = (int(map_center[0]), int(map_center[1]))
        self.have_map_ = True                                                # :63
        if old is not None and getattr(old, "nb", 0):
            self.k.set_polar_table(self.dev, old.nb, old.nr, old.ang_res)

    # top_down_map.cpp:22-31 + 48-58: the static vector map
    def loadVectorMap(self, svg_path, fill_keys, map_center=(0, 0)):
        """Parses svg_path like loadSvg (host), fills the class planes like getRasterMap + getClasses on the GPU
        (tdr_map_load_polygons) and builds the distance maps from them like the constructor (:48-58).  fill_keys[cls]:
        the key of LUT index cls (svg_fill_key(unpackColor(ind2Color(cls)))); params_.flatten_lut / num_classes /
        exclusive_classes / resolution as the reference reads them.  The class planes before the distance transform
        are kept in self.class_planes_ ((ncls, cols, rows) column-major, 0 inside)."""
        import os
        p = self.params_
        if not p.num_classes or not len(p.flatten_lut):
            raise ValueError("Params.num_classes and Params.flatten_lut are needed to load a vector map")
        if len(fill_keys) < len(p.flatten_lut):
            raise ValueError("one fill key per flatten_lut entry is needed")
        if not os.path.exists(svg_path):
            raise FileNotFoundError(svg_path)
        (w, h), polys = parse_svg(svg_path)
        verts, offs, cls = [], [0], []
        for lut_i, flat in enumerate(p.flatten_lut):          # loadSvg :77-103
            if not 0 <= flat < p.num_classes:
                continue
            for key, v in polys:
                if key is not None and key == (int(fill_keys[lut_i]) & 0xFFFFFF):
                    verts.append(v)
                    offs.append(offs[-1] + len(v))
                    cls.append(flat)
        verts = np.concatenate(verts) if verts else np.zeros((0, 2), np.float32)
        planes = self.k.polygon_planes(verts, np.asarray(offs, np.int64), np.asarray(cls, np.int32), int(w), int(h),
                                       p.num_classes, list(p.exclusive_classes), p.resolution)
        # the planes as the raster cache stores them (0 inside, 255 elsewhere, flipped) -> the ingest of loadRasterizedMaps
        raster = np.where(np.transpose(planes, (0, 2, 1)) == 0, 0, 255).astype(np.uint8)[:, ::-1]
        old = self.dev
        self.geo_constant_one_ = False
        self.dev = self.k.make_map_from_rasters(raster, p.resolution)
        self.rows, self.cols = self.dev.rows, self.dev.cols
        self.maps_cm_host, _ = self.k.unpack_map(self.dev)
        self.class_planes_ = planes
        self.map_center_ = (int(map_center[0]), int(map_center[1]))
        self.have_map_ = True                                                # :63
        if old is not None and getattr(old, "nb", 0):
            self.k.set_polar_table(self.dev, old.nb, old.nr, old.ang_res)

    # top_down_map.cpp:32-42 + 48-63: the static colour raster map
    def loadColorRasterMap(self, path_or_bgr, fill_keys, map_center=(0, 0)):
        """The constructor's branch for a colour image: cv::imread (png_read_color for a path; an (H, W, 3) uint8 BGR
        array is taken as decoded), color2Ind against fill_keys (fill_keys[i] = the key of LUT index i,
        svg_fill_key(unpackColor(ind2Color(i)))) and loadCompressedRasterMap + computeDists on the GPU, geometric layers
        derived from the classes like the constructor (:48-58).  have_map_ turns true even without road (:63)."""
        import os
        p = self.params_
        if not p.num_classes or not len(p.flatten_lut):
            raise ValueError("Params.num_classes and Params.flatten_lut are needed to load a colour map")
        if len(fill_keys) < len(p.flatten_lut):
            raise ValueError("one fill key per flatten_lut entry is needed")
        if isinstance(path_or_bgr, (str, bytes, os.PathLike)):
            if not os.path.exists(path_or_bgr):
                raise FileNotFoundError(path_or_bgr)
            bgr = png_read_color(path_or_bgr)
        else:
            bgr = np.ascontiguousarray(path_or_bgr, np.uint8)
            if bgr.ndim != 3 or bgr.shape[2] != 3:
                raise ValueError("loadColorRasterMap needs an (H, W, 3) BGR image")
        old = self.dev
        self.geo_constant_one_ = False
        self.dev = self.k.make_map_from_color(bgr, list(fill_keys)[:len(p.flatten_lut)], p.flatten_lut, p.num_classes,
                                              p.resolution)
        self.rows, self.cols = self.dev.rows, self.dev.cols
        self.maps_cm_host, _ = self.k.unpack_map(self.dev)
        self.map_center_ = (int(map_center[0]), int(map_center[1]))
        self.have_map_ = True                                                # :63
        if old is not None and getattr(old, "nb", 0):
            self.k.set_polar_table(self.dev, old.nb, old.nr, old.ang_res)

    def roadCells(self):
        """The map's road list on the device (include/tdr.h, "recovery injection"): the ascending cell indices
        r * cols + c of the cells the on-road test of particle initialisation accepts.  Built on first use and kept until
        the map's records are written again (every loader and updateMap make a new device map, the incremental update drops
        the list).  A map with fewer than two classes or without a road cell raises."""
        if self.dev is None:
            raise ValueError("roadCells: no map")
        if self.dev.road is None:
            self.dev.road = self.k.road_cells(self.dev)
        if self.dev.road.numel() < 1:
            raise ValueError("roadCells: the map has no road cell")
        return self.dev.road

    # top_down_map.cpp:159-175
    def getClassesAtPoint(self, center):
        cx, cy = center
        res = np.float32(self.params_.resolution)
        if not (isinstance(cx, (int, np.integer)) and isinstance(cy, (int, np.integer))):
            # Vector2f overload (:172-175) converts to an index and then calls the Vector2i overload
            cx, cy = int(np.float32(cx) / res), int(np.float32(cy) / res)
        c0, c1 = int(np.float32(cx) / res), int(np.float32(cy) / res)   # :160
        out = []
        for cls in range(self.params_.num_classes):
            if 0 <= c0 < self.cols and 0 <= c1 < self.rows and self.maps_cm_host[cls, c0, c1] < 1:
                out.append(cls)
        return out

    # top_down_map.cpp:429-459
    def getLocalMap(self, center, rot, res, shape):
        """Cartesian window of one pose: (dists [ncls] list of (rows, cols) arrays, mask (rows, cols) uint8, 1 = unknown
        / outside).  `shape` = (rows, cols) stands for the sizes the reference reads off the caller's arrays."""
        rows, cols = int(shape[0]), int(shape[1])
        d, k = self.k.local_map(self.dev, False, float(center[0]), float(center[1]), float(rot), float(res), rows, cols)
        d = d.cpu().numpy().reshape(self.dev.ncls, cols, rows)
        return [d[c].T.copy() for c in range(self.dev.ncls)], k.cpu().numpy().reshape(cols, rows).T.copy()

    # top_down_map.cpp:461-481
    def getLocalGeoMap(self, center, rot, res, shape):
        """The Cartesian window gathered from the two geometric layers geo_maps_: list of two (rows, cols) arrays."""
        rows, cols = int(shape[0]), int(shape[1])
        g = self.geo_dev()
        d, _ = self.k.local_map(g, False, float(center[0]), float(center[1]), float(rot), float(res), rows, cols)
        d = d.cpu().numpy().reshape(2, cols, rows)
        return [d[c].T.copy() for c in range(2)]

    def geo_dev(self):
        """geo_maps_ on the device (built on first use): derived from the class maps like the static-map constructor does
        (src/top_down_map.cpp:48-58), or the constant 1 the updateMap path leaves (:126-133)."""
        return self.dev.geo_map(self.k, self.geo_constant_one_)

    # --- window (image) shape of the scan the filter scores against -------------------------------------------------
    polar = False

    def setWindow(self, rows, cols):
        """Cartesian window shape (rows = y, cols = x) for the Cartesian score (BASELINE config 4)."""
        self.win_rows, self.win_cols = int(rows), int(cols)

    def window_shape(self):
        return (self.win_rows, self.win_cols)

    def scan_handle(self, scan):
        """Accepts what ParticleFilter::update is handed in the reference (a list of per-class column-major images),
        an (ncls, rows*cols) array / device tensor, or an already packed device scan; returns the packed device scan
        the scoring kernel reads."""
        ncls = self.numClasses()
        nb, nr = self.window_shape()
        if isinstance(scan, tuple) and scan[0] == "pk":
            return scan[1]
        if isinstance(scan, (list, tuple)):
            if len(scan) < ncls:
                raise ValueError("fewer scan images than map classes")
            scan = np.stack([np.asarray(s, np.float32).reshape(nb, nr, order="A").ravel(order="F") for s in scan[:ncls]])
        if isinstance(scan, np.ndarray):
            if scan.shape != (ncls, nb * nr):
                raise ValueError(f"scan shape {scan.shape} != {(ncls, nb * nr)}")
            scan = self.k.to_device(np.ascontiguousarray(scan, np.float32))
        if isinstance(scan, torch.Tensor):
            if tuple(scan.shape) != (ncls, nb * nr):
                raise ValueError(f"scan shape {tuple(scan.shape)} != {(ncls, nb * nr)}")
            return self.k.pack_scan(scan.contiguous(), ncls, nb, nr)
        raise TypeError("unsupported scan type")

    def numClasses(self):
        return self.params_.num_classes

    def size(self):
        return (self.cols, self.rows)

    def mapCenter(self):
        return self.map_center_

    def resolution(self):
        return self.params_.resolution

    def haveMap(self):
        return self.have_map_


class TopDownMapPolar(TopDownMap):
    def __init__(self, params, class_maps=None, class_mask=None, kernels=None):
        super().__init__(params, class_maps, class_mask, kernels)
        if self.have_map_:
            self.samplePtsPolar((100, 50), np.float32(2 * np.pi / 100))   # top_down_map_polar.cpp:3-5

    def samplePtsPolar(self, shape, ang_res):
        """top_down_map_polar.cpp:7-19; shape = (theta bins, range bins)."""
        self.k.set_polar_table(self.dev, int(shape[0]), int(shape[1]), float(ang_res))

    # top_down_map_polar.cpp:21-53 (and the 3-argument overload with scale = 1, :78-81)
    def getLocalMap(self, center, scale_or_res, res=None):   # noqa: D401  (getLocalMap(center, scale, res) / (center, res))
        scale, res = (1.0, scale_or_res) if res is None else (scale_or_res, res)
        d, k = self.k.local_map(self.dev, True, float(center[0]), float(center[1]), float(scale), float(res))
        nb, nr = self.nb, self.nr
        d = d.cpu().numpy().reshape(self.dev.ncls, nr, nb)
        return [d[c].T.copy() for c in range(self.dev.ncls)], k.cpu().numpy().reshape(nr, nb).T.copy()

    # top_down_map_polar.cpp:55-76 (and the 3-argument overload, :83-86)
    def getLocalGeoMap(self, center, scale_or_res, res=None):   # noqa: D401
        scale, res = (1.0, scale_or_res) if res is None else (scale_or_res, res)
        d, _ = self.k.local_map(self.geo_dev(), True, float(center[0]), float(center[1]), float(scale), float(res))
        d = d.cpu().numpy().reshape(2, self.nr, self.nb)
        return [d[c].T.copy() for c in range(2)]

    polar = True

    @property
    def nb(self):
        return self.dev.nb

    @property
    def nr(self):
        return self.dev.nr

    def window_shape(self):
        return (self.nb, self.nr)
