"""GPU: the scan picture, the analog picture and the label picture (include/tdr.h, "the scan picture";
csrc/tdr_scan_viz.hip) against their NumPy restatement (tests/scan_viz_ref.py), byte for byte: the layer-1 launchers and
their job-table forms, the renderer handle, the host-images entry, the Python ScanRenderer, and the label background of
the particle picture."""
import ctypes as C
import math

import numpy as np
import pytest
import scan_viz_ref as S

F32 = np.float32
pytestmark = pytest.mark.gpu
vp = C.c_void_p

# rows x cols: npix = 1, 3, 15, 16, 17, 2500 (the node's), 2145, 65535, 65536 — one pixel, below / at / just above the
# four-pixel run and the 16-byte line of a plane, odd counts (unaligned class planes), more than one workgroup
SHAPES = [(1, 1), (3, 1), (5, 3), (4, 4), (17, 1), (100, 25), (33, 65), (257, 255), (256, 256)]
NCLS = [1, 2, 6, 15]
UNFLATTEN = [3, 200, 17, 255, 0, 9, 31, 32, 33, 64, 65, 127, 128, 129, 254]
LUT = np.random.default_rng(99).integers(0, 256, (256, 3), dtype=np.uint8)


def P(a):
    return a.ctypes.data_as(vp)


@pytest.fixture(scope="module")
def k():
    from top_down_renderer_amd.kernels import HipKernels
    return HipKernels()


@pytest.fixture(scope="module")
def L():
    from top_down_renderer_amd import _lib
    return _lib.load()


def count_case(ncls, npix, seed):
    """Small integer counts, as the renderer produces them: zeros, ties and all-equal pixels are common."""
    return np.random.default_rng(seed).integers(0, 4, (ncls, npix)).astype(F32)


def float_case(ncls, npix, seed):
    """Seeded floats with planted ties (first = last class at the maximum), NaN, +-inf, all-equal and all-NaN pixels."""
    rng = np.random.default_rng(seed)
    a = rng.normal(0, 3, (ncls, npix)).astype(F32)
    for j, p in enumerate(rng.permutation(npix)[: max(1, npix // 3)]):
        kind = j % 7
        if kind == 0:
            a[:, p] = a[0, p]                                  # all equal
        elif kind == 1:
            a[:, p] = np.nan                                   # all NaN
        elif kind == 2:
            a[rng.integers(ncls), p] = np.nan
        elif kind == 3:
            a[rng.integers(ncls), p] = np.inf
        elif kind == 4:
            a[rng.integers(ncls), p] = -np.inf
        elif kind == 5:
            a[0, p] = a[-1, p] = np.abs(a[:, p]).max() + 1     # a tie at the maximum: the last class
        else:
            a[:, p] = np.nan
            a[rng.integers(ncls), p] = 1.0                     # exactly one class is not NaN
    return a


def cases(ncls, npix, seed):
    return [count_case(ncls, npix, seed), float_case(ncls, npix, seed + 1)]


# ---- layer 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncls", NCLS)
def test_scan_picture_launcher(k, ncls):
    import torch
    for si, (rows, cols) in enumerate(SHAPES):
        for ci, imgs in enumerate(cases(ncls, rows * cols, 100 * si + ncls)):
            got = k.scan_picture(k.to_device(imgs), ncls, rows, cols, UNFLATTEN[:ncls], LUT)
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy(), S.scan_picture(imgs, rows, cols, UNFLATTEN[:ncls], LUT)), (rows, cols, ci)


def test_scan_picture_launcher_on_unaligned_buffers(k):
    """Class planes and an output that start off a 16-byte / 4-byte boundary take the scalar loads and byte stores."""
    import torch
    rows, cols, ncls = 33, 65, 6
    imgs = float_case(ncls, rows * cols, 5)
    base = k.zeros((ncls * rows * cols + 1,))
    base[1:] = k.to_device(imgs).reshape(-1)
    out = k.empty((3 * rows * cols + 1,), torch.uint8)
    k.scan_picture(base[1:], ncls, rows, cols, UNFLATTEN[:ncls], LUT, out=out[1:])
    torch.cuda.synchronize()
    assert np.array_equal(out[1:].cpu().numpy().reshape(cols, rows, 3), S.scan_picture(imgs, rows, cols, UNFLATTEN[:ncls], LUT))


ANALOG_VALUES = np.asarray([0, 0.098, 0.1, 0.294, 0.3, 50, 51, -1, np.nan, np.inf, -np.inf, 1e30, -1e30, 0.5, 1.5, 2.5,
                            float.fromhex("0x1.919192p-4"), float.fromhex("0x1.2d2d2ep-2"), float.fromhex("0x1.f5f5f6p-2"),
                            float.fromhex("0x1.f5f5f8p-2"), float.fromhex("0x1.5f5f60p-1")], F32)


def analog_case(npix, scale, seed):
    rng = np.random.default_rng(seed)
    a = (rng.random(npix) * 1.2 * scale).astype(F32)
    # products on and next to the halves, as far as float32 has them
    h = ((rng.integers(0, 256, npix) + 0.5) / (255.0 / scale)).astype(F32)
    a = np.where(rng.random(npix) < 0.3, h, a)
    n = min(npix, len(ANALOG_VALUES))
    a[rng.permutation(npix)[:n]] = ANALOG_VALUES[:n]
    return a


@pytest.mark.parametrize("scale", [1.0, 50.0, 0.37])
def test_analog_picture_launcher(k, scale):
    import torch
    for si, (rows, cols) in enumerate(SHAPES):
        img = analog_case(rows * cols, scale, si)
        got = k.analog_picture(k.to_device(img), rows, cols, scale)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), S.analog_picture(img, rows, cols, scale)), (rows, cols)


def test_analog_hand_values_on_the_device(k):
    import torch
    v = np.resize(ANALOG_VALUES, 24).astype(F32)
    got = k.analog_picture(k.to_device(v), 24, 1, 50.0)
    torch.cuda.synchronize()
    assert got.cpu().numpy()[0, :7, 0].tolist() == [0, 0, 1, 1, 2, 255, 255]
    assert got.cpu().numpy()[0, 7:13, 0].tolist() == [0] * 6
    assert got.cpu().numpy()[0, 16:21, 0].tolist() == [0, 2, 2, 2, 4]           # float32 products on a half: to even


def label_image(H, W, seed):
    """Random labels with every label present (as many as there are cells)."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 256, (H, W), dtype=np.uint8)
    n = min(256, H * W)
    lab.reshape(-1)[rng.permutation(H * W)[:n]] = np.arange(n, dtype=np.uint8)
    return lab


@pytest.mark.parametrize("H,W", [(11, 11), (16, 16), (33, 65), (300, 257)])
def test_label_picture_launcher(k, H, W):
    import torch
    lab = label_image(H, W, H)
    assert H * W < 256 or len(np.unique(lab)) == 256
    got = k.label_picture(k.to_device(lab), LUT)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), S.label_picture(lab, LUT))


def test_job_table_forms(k, L):
    """Three pictures of different sizes in one launch, for each of the three kinds; a bad job writes nothing."""
    import torch
    from top_down_renderer_amd._lib import LabelPictureJobC, ScanPictureJobC, check
    stream = k.stream()
    shapes = [(5, 3, 2), (100, 25, 6), (33, 65, 6), (17, 1, 1)]
    imgs = [float_case(n, r * c, 7 + i) for i, (r, c, n) in enumerate(shapes)]
    dev = [k.to_device(a) for a in imgs]
    outs = [k.empty((c, r, 3), torch.uint8) for r, c, _ in shapes]
    canary = k.empty((64,), torch.uint8)
    canary.fill_(0xA5)
    jobs = (ScanPictureJobC * 5)()
    for i, (r, c, n) in enumerate(shapes):
        jobs[i].imgs, jobs[i].ncls, jobs[i].npix, jobs[i].out_bgr = dev[i].data_ptr(), n, r * c, outs[i].data_ptr()
    jobs[4].imgs, jobs[4].ncls, jobs[4].npix, jobs[4].out_bgr = dev[0].data_ptr(), 7, 15, canary.data_ptr()   # 7 classes > the table's 6
    jobs_dev = k.to_device(np.frombuffer(bytes(jobs), np.uint8).copy())
    unf = np.asarray(UNFLATTEN[:6], np.int32)
    check(L.tdr_k_scan_picture_jobs(jobs_dev.data_ptr(), 5, 2500, P(unf), 6, P(LUT), stream))
    torch.cuda.synchronize()
    for i, (r, c, n) in enumerate(shapes):
        assert np.array_equal(outs[i].cpu().numpy(), S.scan_picture(imgs[i], r, c, UNFLATTEN[:n], LUT)), i
    assert (canary.cpu().numpy() == 0xA5).all()
    # analog: the first layer of each
    check(L.tdr_k_analog_picture_jobs(jobs_dev.data_ptr(), 4, 2500, C.c_float(0.37), stream))
    torch.cuda.synchronize()
    for i, (r, c, n) in enumerate(shapes):
        assert np.array_equal(outs[i].cpu().numpy(), S.analog_picture(imgs[i][0], r, c, 0.37)), i
    # labels
    labs = [label_image(11, 11, 1), label_image(33, 65, 2), label_image(300, 257, 3)]
    ldev = [k.to_device(a) for a in labs]
    louts = [k.empty(a.shape + (3,), torch.uint8) for a in labs]
    lj = (LabelPictureJobC * 3)()
    for i, a in enumerate(labs):
        lj[i].labels, lj[i].npix, lj[i].out_bgr = ldev[i].data_ptr(), a.size, louts[i].data_ptr()
    lj_dev = k.to_device(np.frombuffer(bytes(lj), np.uint8).copy())
    check(L.tdr_k_label_picture_jobs(lj_dev.data_ptr(), 3, 300 * 257, P(LUT), stream))
    torch.cuda.synchronize()
    for i, a in enumerate(labs):
        assert np.array_equal(louts[i].cpu().numpy(), S.label_picture(a, LUT)), i


def test_launchers_refuse_bad_arguments_before_any_launch(k, L):
    import torch
    img = k.zeros((64,))
    out = k.empty((64,), torch.uint8)
    out.fill_(0xA5)
    unf = np.asarray(UNFLATTEN, np.int32)
    ip, op, s = img.data_ptr(), out.data_ptr(), k.stream()
    bad = [L.tdr_k_scan_picture(None, 2, 8, P(unf), P(LUT), op, s), L.tdr_k_scan_picture(ip, 2, 8, None, P(LUT), op, s),
           L.tdr_k_scan_picture(ip, 2, 8, P(unf), None, op, s), L.tdr_k_scan_picture(ip, 2, 8, P(unf), P(LUT), None, s),
           L.tdr_k_scan_picture(ip, 0, 8, P(unf), P(LUT), op, s), L.tdr_k_scan_picture(ip, 16, 4, P(unf), P(LUT), op, s),
           L.tdr_k_scan_picture(ip, 2, 0, P(unf), P(LUT), op, s),
           L.tdr_k_analog_picture(None, 8, C.c_float(1), op, s), L.tdr_k_analog_picture(ip, 0, C.c_float(1), op, s),
           L.tdr_k_analog_picture(ip, 8, C.c_float(0), op, s), L.tdr_k_analog_picture(ip, 8, C.c_float(-1), op, s),
           L.tdr_k_analog_picture(ip, 8, C.c_float(math.nan), op, s), L.tdr_k_analog_picture(ip, 8, C.c_float(math.inf), op, s),
           L.tdr_k_label_picture(None, 8, P(LUT), op, s), L.tdr_k_label_picture(op, 8, None, op, s),
           L.tdr_k_label_picture(op, 0, P(LUT), op, s),
           L.tdr_k_scan_picture_jobs(ip, 0, 8, P(unf), 6, P(LUT), s), L.tdr_k_scan_picture_jobs(None, 1, 8, P(unf), 6, P(LUT), s),
           L.tdr_k_scan_picture_jobs(ip, 1, 8, P(unf), 16, P(LUT), s), L.tdr_k_analog_picture_jobs(ip, 0, 8, C.c_float(1), s),
           L.tdr_k_analog_picture_jobs(ip, 1, 8, C.c_float(0), s), L.tdr_k_label_picture_jobs(ip, 0, 8, P(LUT), s),
           L.tdr_k_label_picture_jobs(ip, 1, 8, None, s)]
    assert bad == [-1] * len(bad)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all()


# ---- the renderer handle, the host-images entry, the Python ScanRenderer ----------------------------------------------------
def cloud(n, reach, nlabels, seed):
    """(n, 8) pcl::PointXYZI-strided points within `reach` of the origin, the label at float 4."""
    rng = np.random.default_rng(seed)
    pts = np.zeros((n, 8), F32)
    pts[:, :2] = rng.uniform(-reach, reach, (n, 2))
    pts[:, 2] = rng.uniform(-1, 1, n)
    pts[:, 4] = rng.integers(0, nlabels, n)
    return pts


def flatten_lut(ncls):
    return (np.arange(256) % ncls).astype(np.int32)


def render_layout(img):
    """(ncls, rows, cols) images as get_render returns them -> [ncls][rows*cols] column-major."""
    return np.ascontiguousarray(np.transpose(img, (0, 2, 1))).reshape(img.shape[0], -1)


@pytest.mark.parametrize("polar", [True, False])
@pytest.mark.parametrize("ncls", NCLS)
def test_renderer_handle_and_host_images_entry(L, polar, ncls):
    from top_down_renderer_amd import batch
    from top_down_renderer_amd._lib import check
    r = batch.Renderer(flatten_lut(ncls))
    for si, (rows, cols) in enumerate(SHAPES):
        pts = cloud(400, 0.4 * cols if polar else 0.4 * max(rows, cols), 2 * ncls, si)
        if polar:
            r.render_polar(pts, 8, 4, 1.0, 2 * math.pi / rows, ncls, rows, cols)
        else:
            r.render_cart(pts, 8, 4, 1.0, ncls, rows, cols)
        img, _ = r.get_render()
        imgs = render_layout(img)
        if rows * cols > 16 and ncls > 1:
            assert imgs.max() > 0                                                       # the cloud did land in the image
        want = S.scan_picture(imgs, rows, cols, UNFLATTEN[:ncls], LUT)
        assert np.array_equal(r.picture(UNFLATTEN[:ncls], LUT), want), (rows, cols)     # tdr_renderer_visualize
        for c in {0, ncls - 1}:
            assert np.array_equal(r.picture_analog(c, 0.37), S.analog_picture(imgs[c], rows, cols, 0.37)), (rows, cols, c)
        # the same images from the host, and the float case
        unf = np.asarray(UNFLATTEN[:ncls], np.int32)
        for a in (imgs, float_case(ncls, rows * cols, si)):
            a = np.ascontiguousarray(a, F32)
            out = np.zeros((cols, rows, 3), np.uint8)
            check(L.tdr_scan_picture_host(P(a), ncls, rows, cols, P(unf), P(LUT), P(out)))
            assert np.array_equal(out, S.scan_picture(a, rows, cols, unf, LUT)), (rows, cols)


@pytest.mark.parametrize("scale", [1.0, 50.0, 0.37])
def test_renderer_handle_analog_scales(scale):
    from top_down_renderer_amd import batch
    ncls = 6
    r = batch.Renderer(flatten_lut(ncls))
    for si, (rows, cols) in enumerate(SHAPES):
        r.render_polar(cloud(3000, 0.3 * cols, 2 * ncls, si), 8, 4, 1.0, 2 * math.pi / rows, ncls, rows, cols)
        imgs = render_layout(r.get_render()[0])
        assert np.array_equal(r.picture_analog(2, scale), S.analog_picture(imgs[2], rows, cols, scale)), (rows, cols)


def test_renderer_handle_after_a_batched_render():
    from top_down_renderer_amd import batch
    ncls, nb, nr = 6, 100, 25
    rs = [batch.Renderer(flatten_lut(ncls)) for _ in range(3)]
    clouds = [(cloud(500 * (i + 1), 10.0, 12, 40 + i), 8, 4) for i in range(3)]
    batch.render_batch(rs, clouds, 1.0, 2 * math.pi / nb, ncls, nb, nr)
    pics = [r.picture(UNFLATTEN[:ncls], LUT) for r in rs]                              # ordered after the batched render
    for r, pic in zip(rs, pics):
        imgs = render_layout(r.get_render()[0])
        assert imgs.max() > 0
        assert np.array_equal(pic, S.scan_picture(imgs, nb, nr, UNFLATTEN[:ncls], LUT))
    batch.render_batch(rs, clouds[::-1], 1.0, 2 * math.pi / nb, ncls, nb, nr)         # and a render after the pictures
    for r in rs:
        assert np.array_equal(r.picture(UNFLATTEN[:ncls], LUT),
                              S.scan_picture(render_layout(r.get_render()[0]), nb, nr, UNFLATTEN[:ncls], LUT))


@pytest.mark.parametrize("polar", [True, False])
def test_python_scan_renderer(k, polar):
    import top_down_renderer_amd as pkg
    ncls = 6
    r = (pkg.ScanRendererPolar if polar else pkg.ScanRenderer)(flatten_lut(ncls), kernels=k)
    with pytest.raises(ValueError, match="no render"):
        r.renderViz(UNFLATTEN[:ncls], LUT)
    for si, (rows, cols) in enumerate(SHAPES):
        r.set_output_shape(ncls, rows, cols)
        pts = cloud(2000, 0.4 * cols if polar else 0.4 * max(rows, cols), 12, si)
        if polar:
            r.renderSemanticTopDown(pts, 1.0, 2 * math.pi / rows)
        else:
            r.renderSemanticTopDown(pts, 1.0)
        imgs = r.last_images().cpu().numpy().reshape(ncls, rows * cols)
        assert np.array_equal(r.renderViz(UNFLATTEN[:ncls], LUT), S.scan_picture(imgs, rows, cols, UNFLATTEN[:ncls], LUT)), (rows, cols)
        assert np.array_equal(r.renderVizAnalog(1, 0.37), S.analog_picture(imgs[1], rows, cols, 0.37)), (rows, cols)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            r.renderVizAnalog(0, bad)
    with pytest.raises(ValueError):
        r.renderVizAnalog(ncls, 1.0)


def test_renderer_refusals_leave_the_output_untouched(L):
    from top_down_renderer_amd import batch
    ncls, rows, cols = 6, 33, 65
    r = batch.Renderer(flatten_lut(ncls))
    unf = np.asarray(UNFLATTEN[:ncls], np.int32)
    out = np.full((cols, rows, 3), 0xA5, np.uint8)
    oh, ow = C.c_int(-7), C.c_int(-7)

    def refused(rc, word):
        assert rc == -1 and word in L.tdr_last_error().decode(), L.tdr_last_error()
        assert (out == 0xA5).all()

    refused(L.tdr_renderer_visualize(r.h, P(unf), P(LUT), P(out), out.size, C.byref(oh), C.byref(ow)), "no render")
    refused(L.tdr_renderer_visualize_analog(r.h, 0, C.c_float(1.0), P(out), out.size, C.byref(oh), C.byref(ow)), "no render")
    assert (oh.value, ow.value) == (-7, -7)
    r.render_polar(cloud(500, 20.0, 12, 3), 8, 4, 1.0, 2 * math.pi / rows, ncls, rows, cols)
    refused(L.tdr_renderer_visualize(r.h, P(unf), P(LUT), P(out), out.size - 1, C.byref(oh), C.byref(ow)), "room")
    assert (oh.value, ow.value) == (cols, rows)                                        # the size is still reported
    refused(L.tdr_renderer_visualize_analog(r.h, 0, C.c_float(1.0), P(out), out.size - 1, C.byref(oh), C.byref(ow)), "room")
    for bad in (0.0, -2.0, math.nan, math.inf):
        refused(L.tdr_renderer_visualize_analog(r.h, 0, C.c_float(bad), P(out), out.size, C.byref(oh), C.byref(ow)), "scale")
    refused(L.tdr_renderer_visualize_analog(r.h, ncls, C.c_float(1.0), P(out), out.size, C.byref(oh), C.byref(ow)), "class")
    refused(L.tdr_renderer_visualize(r.h, None, P(LUT), P(out), out.size, C.byref(oh), C.byref(ow)), "null")
    refused(L.tdr_scan_picture_host(None, ncls, rows, cols, P(unf), P(LUT), P(out)), "null")
    refused(L.tdr_scan_picture_host(P(np.zeros(4, F32)), 16, 2, 2, P(unf), P(LUT), P(out)), "shape")
    assert L.tdr_renderer_visualize(r.h, P(unf), P(LUT), P(out), out.size, C.byref(oh), C.byref(ow)) == 0   # and it still draws
    assert not (out == 0xA5).all()


# ---- the label background of the particle picture -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    from top_down_renderer_amd import synth
    return synth.make_scene("c1", n_particles=512)


def test_label_background_equals_the_host_coloured_one(k, scene, L):
    import test_viz as TV
    sc = scene
    H, W = sc.class_maps.shape[1:]
    a, b = TV.Handle(sc, len(sc.states)), TV.Handle(sc, len(sc.states))
    try:
        for h in (a, b):
            h.set_states(sc.states)
        arrows = [[10, 10, 40, 30]]
        for hh, ww in ((H, W), (11, 11), (37, 300)):          # a second and a third background replace the first
            lab = label_image(hh, ww, hh)
            assert a.set_background(S.label_picture(lab, LUT)) == 0
            assert L.tdr_filter_set_viz_background_labels(b.f, P(lab), hh, ww, P(LUT)) == 0
            for s in (1.0, 0.37):
                (rca, ia), (rcb, ib) = a.visualize(s, arrows), b.visualize(s, arrows)
                assert rca == 0 and rcb == 0 and ia.shape == ib.shape and np.array_equal(ia, ib), (hh, ww, s)
        # the same size limits
        small = np.zeros((10, 40), np.uint8)
        assert L.tdr_filter_set_viz_background_labels(b.f, P(small), 10, 40, P(LUT)) == -1
        assert "10 x 40" in L.tdr_last_error().decode()
        assert L.tdr_filter_set_viz_background_labels(b.f, P(small), 40, 10, P(LUT)) == -1
        assert L.tdr_filter_set_viz_background_labels(b.f, None, 40, 40, P(LUT)) == -1
        assert L.tdr_filter_set_viz_background_labels(b.f, P(small), 40, 40, None) == -1
        assert np.array_equal(a.visualize(1.0)[1], b.visualize(1.0)[1])          # the refusals changed nothing
        # the Python filter
        f, r, m = TV.python_filter(k, sc)
        lab = label_image(H, W, 5)
        f.setVizBackground(labels=lab, lut=LUT)
        pic = f.renderViz(0.5, arrows)
        f.setVizBackground(S.label_picture(lab, LUT))
        assert np.array_equal(pic, f.renderViz(0.5, arrows))
    finally:
        a.close()
        b.close()
