"""Builds libtdr_hip.so (HIP kernels + C ABI) in-tree for gfx950 with hipcc.  No GPU is needed to compile.

Every translation unit is compiled to an object of its own (in parallel; only those whose source or headers changed) and
the objects are linked into the shared library."""
import glob
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
SRC = [os.path.join(PKG, "csrc", f) for f in
       ("tdr_core.hip", "tdr_map.hip", "tdr_raster.hip", "tdr_score.hip", "tdr_score_init.hip", "tdr_score_su.hip", "tdr_score_ray.hip", "tdr_score_cart.hip", "tdr_score_cart_init.hip", "tdr_filter.hip", "tdr_rng.hip", "tdr_prefix.hip",
        "tdr_geo.hip", "tdr_cmap.hip", "tdr_active.hip", "tdr_poly.hip", "tdr_batch.hip", "tdr_batch_loop.hip", "tdr_init.hip", "tdr_map_incr.hip", "tdr_viz.hip", "tdr_scan_viz.hip", "tdr_gmm.hip", "tdr_fuse.hip", "tdr_kld.hip", "tdr_recover.hip", "tdr_recover_sensor.hip", "tdr_grid.hip", "tdr_eig.cpp", "tdr_host_map.cpp", "tdr_host_map_load.cpp", "tdr_host_renderer.cpp", "tdr_host_filter.cpp",
        "tdr_host_batch.cpp", "tdr_host_gmm.cpp", "tdr_host_fuse.cpp", "tdr_host_kld.cpp", "tdr_host_recover.cpp", "tdr_host_grid.cpp", "tdr_host_selftest.cpp", "tdr_config.cpp", "tdr_comm.cpp", "tdr_gmm.cpp", "tdr_png.cpp",
        "tdr_svg.cpp")]
# every header: a changed one rebuilds every translation unit (no per-file dependency tracking)
HDR = [os.path.join(ROOT, "include", "tdr.h")] + sorted(glob.glob(os.path.join(PKG, "csrc", "*.h")))
OUT = os.path.join(PKG, "libtdr_hip.so")
OBJ_DIR = os.path.join(PKG, "_obj")
STAMP = os.path.join(PKG, "libtdr_hip.toolchain.txt")

# -ffp-contract=off: index arithmetic must round like the reference's non-FMA x86-64 build (see csrc/tdr_common.h)
CFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-I", os.path.join(ROOT, "include")]
LDFLAGS = ["--offload-arch=gfx950", "-shared", "-fPIC", "-ldl", "-lz"]   # zlib: the PNG files of the raster cache
# per-file flags.  tdr_score_init.hip: matrix-core accumulators in VGPRs — with AGPR accumulators the register allocator rotates
# the six accumulator tiles of the init-search loop through ~36 v_accvgpr moves per step (there is no register pressure:
# 112 VGPRs at 4 waves per SIMD)
FILE_FLAGS = {"tdr_score_init.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"],
              # wave-uniform branch trees stay plain scalar branches (see the file's header comment)
              "tdr_score_su.hip": ["-mllvm", "-structurizecfg-skip-uniform-regions"],
              "tdr_score_cart.hip": ["-mllvm", "-structurizecfg-skip-uniform-regions"]}


def hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the HIP extension cannot be built (there is no CPU fallback)")
    return exe


def _obj(src):
    return os.path.join(OBJ_DIR, os.path.basename(src) + ".o")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def needs_build():
    return _stale(OUT, SRC + HDR + [os.path.abspath(__file__)])


def build(force=False, verbose=False, extra_flags=()):
    if not force and not needs_build():
        return OUT
    os.makedirs(OBJ_DIR, exist_ok=True)
    cc = hipcc()
    todo = [s for s in SRC if force or extra_flags or _stale(_obj(s), [s] + HDR + [os.path.abspath(__file__)])]

    def compile_one(src):
        cmd = [cc] + CFLAGS + FILE_FLAGS.get(os.path.basename(src), []) + list(extra_flags) + \
              ["-c", "-x", "hip", src, "-o", _obj(src)]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)

    with ThreadPoolExecutor(max_workers=min(8, max(1, len(todo)))) as ex:
        list(ex.map(compile_one, todo))
    cmd = [cc] + LDFLAGS + ["-o", OUT] + [_obj(s) for s in SRC]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    # build stamp: the toolchain the objects came from.  Two kernels issue loads through inline assembly with hand-counted
    # waits (tdr_score_su_asm.h, tdr_score_cart.hip): their correctness leans on this compiler's register allocation, the
    # bit-parity tests are the guard, and the stamp says which compiler the guard last passed with (bench.py reports it).
    try:
        ver = subprocess.run([cc, "--version"], capture_output=True, text=True).stdout.strip().splitlines()
        open(STAMP, "w").write("\n".join(ver[:3]) + "\n")
    except OSError:
        pass
    return OUT


def toolchain():
    """First line of the build stamp (hipcc --version at build time), or None."""
    try:
        return open(STAMP).read().splitlines()[0]
    except OSError:
        return None


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="-v" in sys.argv))
