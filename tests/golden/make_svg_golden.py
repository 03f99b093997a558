"""Regenerates tests/golden/svg_nanosvg.npz: what the reference's own SVG reader makes of the fixtures in tests/golden/svg/.

The reference (KumarRobotics/top_down_renderer) parses its static map with nanosvg, a single C header it vendors
(include/top_down_render/nanosvg.h), and keeps per shape and subpath the polygon of TopDownMap::loadSvg
(src/top_down_map.cpp:66-110): the points pts[0], pts[3], ... while i < npts - 1, as (x, height - y).  This script
compiles a small driver written for this project against that header, in a temporary directory outside the repository,
runs it on every fixture and stores, per fixture:
    <name>/size   float32 [2]     the image's float width / height
    <name>/keys   uint32 [P]      per polygon: fill.color & 0xFFFFFF (0xFFFFFFFF for a gradient paint)
    <name>/offs   int64 [P + 1]   vertex offsets
    <name>/verts  float32 [V, 2]  vertices
Usage: python tests/golden/make_svg_golden.py [--reference DIR]   (DIR: a checkout of the reference; default: the
TDR_REFERENCE environment variable, else a `reference` directory beside this repository).  Only the .npz is committed;
no test reads the reference.
"""
import argparse
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SVG_DIR = os.path.join(HERE, "svg")
OUT = os.path.join(HERE, "svg_nanosvg.npz")

DRIVER = r"""
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#define NANOSVG_IMPLEMENTATION
#include "top_down_render/nanosvg.h"

/* loadSvg's loop over every shape (no colour filter: the key is written instead), binary to stdout */
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  NSVGimage* img = nsvgParseFromFile(argv[1], "px", 96);
  if (!img) return 1;
  fwrite(&img->width, 4, 1, stdout);
  fwrite(&img->height, 4, 1, stdout);
  for (NSVGshape* s = img->shapes; s; s = s->next) {
    uint32_t key = (s->fill.type == NSVG_PAINT_LINEAR_GRADIENT || s->fill.type == NSVG_PAINT_RADIAL_GRADIENT)
                       ? 0xFFFFFFFFu : (s->fill.color & 0xFFFFFFu);
    for (NSVGpath* p = s->paths; p; p = p->next) {
      int64_t n = 0;
      for (int i = 0; i < p->npts - 1; i += 3) n++;
      fwrite(&key, 4, 1, stdout);
      fwrite(&n, 8, 1, stdout);
      for (int i = 0; i < p->npts - 1; i += 3) {
        float v[2] = {p->pts[i * 2], img->height - p->pts[i * 2 + 1]};
        fwrite(v, 4, 2, stdout);
      }
    }
  }
  nsvgDelete(img);
  return 0;
}
"""


def parse_driver_output(buf):
    w, h = struct.unpack_from("<ff", buf, 0)
    at = 8
    keys, offs, verts = [], [0], []
    while at < len(buf):
        key, n = struct.unpack_from("<Iq", buf, at)
        at += 12
        v = np.frombuffer(buf, np.float32, 2 * n, at).reshape(n, 2)
        at += 8 * n
        keys.append(key)
        verts.append(v)
        offs.append(offs[-1] + n)
    verts = np.concatenate(verts) if verts else np.zeros((0, 2), np.float32)
    return (np.array([w, h], np.float32), np.array(keys, np.uint32), np.array(offs, np.int64),
            np.ascontiguousarray(verts, np.float32))


def save_npz(path, arrays):
    """np.savez with fixed member timestamps: the same fixtures give the same bytes."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as zf:
        for k in sorted(arrays):
            bio = io.BytesIO()
            np.lib.format.write_array(bio, np.asanyarray(arrays[k]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), bio.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TDR_REFERENCE",
                                                          os.path.join(os.path.dirname(ROOT), "reference")))
    args = ap.parse_args()
    inc = os.path.join(args.reference, "include")
    if not os.path.exists(os.path.join(inc, "top_down_render", "nanosvg.h")):
        sys.exit(f"nanosvg.h not found under {inc}: pass --reference")
    tmp = tempfile.mkdtemp(prefix="tdr_svg_golden_")
    try:
        src, exe = os.path.join(tmp, "driver.c"), os.path.join(tmp, "driver")
        open(src, "w").write(DRIVER)
        # the reference's x86-64 build: no FMA contraction
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-I", inc, src, "-o", exe, "-lm"], check=True)
        out = {}
        for name in sorted(os.listdir(SVG_DIR)):
            if not name.endswith(".svg"):
                continue
            buf = subprocess.run([exe, os.path.join(SVG_DIR, name)], check=True, capture_output=True).stdout
            size, keys, offs, verts = parse_driver_output(buf)
            stem = name[:-4]
            out[f"{stem}/size"], out[f"{stem}/keys"], out[f"{stem}/offs"], out[f"{stem}/verts"] = size, keys, offs, verts
            print(f"{name}: {size[0]} x {size[1]}, {len(keys)} polygons, {len(verts)} vertices")
        save_npz(OUT, out)
        print("wrote", OUT)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
