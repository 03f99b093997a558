"""NumPy restatement of the scan picture, the analog picture and the label picture (include/tdr.h, "the scan picture"),
written from the reference's text (src/top_down_render.cpp:266-305, :584) and the rules stated there.

`imgs` is the render layout [ncls][rows*cols] (or [ncls][cols][rows]: column-major Eigen arrays, element (i, j) at
i + j*rows).  A picture is uint8 [cols][rows][3], BGR: pixel (y, x) shows Eigen element (x, y)."""
import numpy as np

F32 = np.float32


def labels(imgs, unflatten):
    """[npix] uint8 labels of a [ncls][npix] stack: the reference's loop, comparison for comparison."""
    imgs = np.asarray(imgs, F32)
    ncls, npix = imgs.shape
    best = np.full(npix, -np.inf, F32)
    worst = np.full(npix, np.inf, F32)
    best_cls = np.full(npix, 255, np.int64)
    with np.errstate(invalid="ignore"):
        for c in range(ncls):
            v = imgs[c]
            ge = v >= best                      # False for a NaN
            best = np.where(ge, v, best)
            best_cls = np.where(ge, c, best_cls)
            worst = np.where(v < worst, v, worst)
    table = np.concatenate([np.asarray(unflatten, np.int64)[:ncls] & 255, np.full(256 - ncls, 255, np.int64)])
    unknown = (best == worst) | (best_cls == 255)
    return np.where(unknown, 255, table[best_cls]).astype(np.uint8)


def scan_picture(imgs, rows, cols, unflatten, lut_bgr):
    imgs = np.asarray(imgs, F32).reshape(-1, rows * cols)
    lut = np.asarray(lut_bgr, np.uint8).reshape(256, 3)
    return lut[labels(imgs, unflatten)].reshape(cols, rows, 3)


def grey(values, scale):
    """uint8 grey of float32 values: lrintf(v * (float)(255.0 / scale)) clamped, 0 where the product does not convert."""
    v = np.asarray(values, F32)
    a = F32(255.0 / float(F32(scale)))
    with np.errstate(invalid="ignore", over="ignore"):
        t = (v * a).astype(F32)
        ok = (t >= F32(-2147483648.0)) & (t < F32(2147483648.0))     # False for NaN and the infinities
        r = np.rint(np.where(ok, t, F32(0)).astype(np.float64))        # half to even; exact in double
    return np.where(ok, np.clip(r, 0, 255), 0).astype(np.uint8)


def analog_picture(img, rows, cols, scale):
    g = grey(np.asarray(img, F32).reshape(rows * cols), scale)
    return np.repeat(g[:, None], 3, axis=1).reshape(cols, rows, 3)


def label_picture(label_img, lut_bgr):
    return np.asarray(lut_bgr, np.uint8).reshape(256, 3)[np.asarray(label_img, np.uint8)]
