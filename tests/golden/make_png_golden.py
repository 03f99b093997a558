"""Writes the colour PNG fixtures of tests/test_color_map.py: tests/golden/png/<name>.png, written by PIL in the PNG
modes a colour map may come in, and tests/golden/png_bgr.npz, the BGR8 image cv::imread gives for each (key = name).

The expected images come from PIL's own decoder, not from the library: convert("RGB") drops alpha without compositing,
expands palettes (ignoring transparency) and replicates grey, which is what OpenCV's libpng set-up does for 8-bit
samples; for the 16-bit greyscale file the expected value is the high byte of each sample (png_set_strip_16).  PIL
writes neither interlaced files nor 16-bit colour: tests/test_color_map.py's own encoder covers those.

    python tests/golden/make_png_golden.py
"""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "png")


def main():
    rng = np.random.default_rng(7)
    os.makedirs(OUT, exist_ok=True)
    H, W = 13, 21   # odd sizes: rows of sub-byte samples end in padding bits
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    alpha = rng.integers(0, 256, (H, W), dtype=np.uint8)
    grey = rng.integers(0, 256, (H, W), dtype=np.uint8)
    files = {
        "l": Image.fromarray(grey, "L"),
        "la": Image.fromarray(np.dstack([grey, alpha]), "LA"),
        "rgb": Image.fromarray(rgb, "RGB"),
        "rgba": Image.fromarray(np.dstack([rgb, alpha]), "RGBA"),
        "bilevel": Image.fromarray(grey > 127).convert("1"),
    }
    save_kw = {}
    for bits in (1, 2, 4, 8):   # palette images at every bit depth, a palette of fewer entries than the depth allows
        n = min(1 << bits, 200)
        pal = rng.integers(0, 256, (n, 3), dtype=np.uint8)
        idx = rng.integers(0, n, (H, W), dtype=np.uint8)
        im = Image.fromarray(idx, "P")
        im.putpalette(pal.ravel().tolist())
        files[f"p{bits}"] = im
        save_kw[f"p{bits}"] = {"bits": bits}
    g16 = rng.integers(0, 65536, (H, W), dtype=np.uint16)
    files["l16"] = Image.fromarray(g16.astype(np.int32), "I").convert("I;16")
    expected = {}
    for name, im in files.items():
        path = os.path.join(OUT, name + ".png")
        im.save(path, optimize=False, **save_kw.get(name, {}))
        back = Image.open(path)
        if name == "l16":
            expected[name] = np.repeat((np.asarray(back, np.uint16) >> 8).astype(np.uint8)[..., None], 3, axis=2)
        else:
            expected[name] = np.ascontiguousarray(np.asarray(back.convert("RGB"))[..., ::-1])
    np.savez_compressed(os.path.join(HERE, "png_bgr.npz"), **expected)


if __name__ == "__main__":
    main()
