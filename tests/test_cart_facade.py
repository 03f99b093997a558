"""The C++ construction path of a Cartesian filter (include/top_down_render/particle_filter_cartesian.h,
TopDownMap::setWindow): tests/cpp/facade_cart.cpp is built against the headers under -Wall -Werror and run on values
dumped here from the Python ParticleFilter on the same map, seed and scans — a cold-start update and a steady-state step
must end with the same bytes."""
import os
import subprocess
import tempfile

import numpy as np
import pytest
from cart_ref import CASES, make_case

from top_down_renderer_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def facade_cart_exe():
    from top_down_renderer_amd import build
    build.build()
    pkg = os.path.join(ROOT, "top_down_renderer_amd")
    exe = os.path.join(tempfile.mkdtemp(prefix="tdr_facade_"), "facade_cart")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "facade_cart.cpp"), "-o", exe, "-L", pkg, "-ltdr_hip",
                    f"-Wl,-rpath,{pkg}"], check=True)
    return exe


def test_facade_cart_compiles(facade_cart_exe):
    assert os.access(facade_cart_exe, os.X_OK)


def test_existing_call_sites_compile_next_to_the_cartesian_header():
    """tests/cpp/call_sites.cpp, unchanged, with particle_filter_cartesian.h force-included in front of it."""
    with tempfile.TemporaryDirectory(prefix="tdr_call_sites_") as tmp:
        subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-include", "top_down_render/particle_filter_cartesian.h",
                        os.path.join(ROOT, "tests", "cpp", "call_sites.cpp")], check=True, cwd=tmp)


@pytest.mark.gpu
def test_facade_cart_matches_the_python_filter(facade_cart_exe):
    import top_down_renderer_amd as pkg
    from oracle import c_oracle as oracle
    from top_down_renderer_amd.kernels import HipKernels
    k = HipKernels()
    name = "c6_32x24"
    ncls, rows, cols, _ = CASES[name]
    cfg, lab, maps, mask, pose, pts, st = make_case(name)
    st = st[2:130].copy()
    st["scale"] = 1.0
    st["have_init"] = 0
    st["theta"] = 0
    n, seed = len(st), 21
    scan0 = oracle.raster_cart(pts, cfg.res, synth.make_lut(ncls), ncls, rows, cols)
    scan1 = np.ascontiguousarray(scan0 + (np.random.default_rng(4).integers(0, 6, scan0.shape) == 0), np.float32)
    motion = np.asarray([cfg.res, 0.4, 0.1, 0.02], np.float32)
    m = pkg.TopDownMap(pkg.Params(resolution=1.0), maps, mask, kernels=k)
    m.setWindow(rows, cols)
    f = pkg.ParticleFilter(n, m, pkg.FilterParams(fixed_scale=1.0), seed=seed, kernels=k, init_particles=False)
    f.set_states(st)
    path = os.path.join(tempfile.mkdtemp(prefix="tdr_facade_"), "cart.bin")
    with open(path, "wb") as fh:
        fh.write(np.asarray([ncls, maps.shape[1], maps.shape[2], rows, cols, n, seed], np.int32).tobytes())
        fh.write(np.ascontiguousarray(np.transpose(maps, (0, 2, 1)), np.float32).tobytes())
        fh.write(np.ascontiguousarray(mask.T, np.uint8).tobytes())
        fh.write(st.tobytes())
        fh.write(scan0.tobytes() + scan1.tobytes() + motion.tobytes())
        for step, scan in enumerate((scan0, scan1)):
            if step:
                f.propagate((float(motion[1]), float(motion[2])), float(motion[3]))
            f.update(np.ascontiguousarray(scan), None, float(motion[0]))
            fh.write(f.get_states().tobytes() + f.raw_weights().tobytes() + f.weights().tobytes())
    out = subprocess.run([facade_cart_exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["ok", str(n)], out.stdout
