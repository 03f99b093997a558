"""tdr_gmm_candidates_host (csrc/tdr_gmm.hip, host code: runs without a GPU): the fits the device path makes for one
filter — k, k + 1, k - 1 — against the branch conditions of the oracle's gmm_select (oracle/np_oracle.py, the NumPy
statement of tdr_gmm_select_host's search, src/particle_filter.cpp:259, 276-297)."""
import ctypes as C

import numpy as np
import pytest

from oracle import np_oracle as no
from top_down_renderer_amd import _lib


def _oracle_branches(monkeypatch, n, k0, m, max_k=32):
    """Which fits gmm_select asks for before it decides: its own code runs, with the fit replaced by a recorder."""
    calls = []

    def fit(X, k, *a, **kw):
        calls.append(k)
        return np.zeros(k), np.zeros((k, 4)), np.zeros((k, 4, 4)), 0.0

    monkeypatch.setattr(no, "gmm_fit", fit)
    no.gmm_select(np.zeros((m, 4)), n, k0, max_k)
    k, tried = calls[0], calls[1:-1]      # (the last call is the refit at the chosen count)
    return [k, k + 1 if k + 1 in tried else 0, k - 1 if k - 1 in tried else 0]


@pytest.mark.parametrize("m", [1, 2, 37, 1000])
def test_candidates_follow_the_selection_rule_s_branch_conditions(monkeypatch, m):
    lib = _lib.load()
    for n in (1, 19, 20, 40, 99, 100, 101, 20000):
        for k0 in (1, 2, 5, 32, 33):
            cand = (C.c_int * 3)(-1, -1, -1)
            assert lib.tdr_gmm_candidates_host(k0, n, m, 32, cand) == 0
            assert list(cand) == _oracle_branches(monkeypatch, n, k0, m), (n, k0, m)
            assert 1 <= cand[0] <= min(32, m) and cand[1] <= min(32, m)


def test_candidates_refuse_bad_arguments():
    lib = _lib.load()
    cand = (C.c_int * 3)()
    assert lib.tdr_gmm_candidates_host(1, 100, 0, 32, cand) != 0
    assert lib.tdr_gmm_candidates_host(1, 100, 10, 0, cand) != 0
    assert lib.tdr_gmm_candidates_host(1, 100, 10, 32, None) != 0
    assert lib.tdr_gmm_out_doubles(3) == 65 and lib.tdr_gmm_workspace_bytes(1000, 32) == 256000


def test_node_loop_program_and_class_methods_compile():
    """tests/cpp/facade_gmm.cpp (run by tests/test_gmm_device.py on the GPU) and the classes' device-fit methods."""
    import os
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tempfile.mkdtemp(prefix="tdr_gmm_hdr_")
    src = os.path.join(d, "hdr.cpp")
    open(src, "w").write('#include "top_down_render/tdr_compat.h"\n#include "top_down_render/particle_filter_cartesian.h"\n'
                         '#include "top_down_render/top_down_render_core_batch.h"\n'
                         "void f(ParticleFilterCartesian* c, ParticleFilter* p) {\n"
                         "  c->computeGMMDevice(); p->computeGMMDevice(); ParticleFilterBatch b; b.computeGMM({p});\n"
                         "  TopDownRenderCore::Config cfg; cfg.gmm_every = 2; }\n")
    for s in (src, os.path.join(root, "tests", "cpp", "facade_gmm.cpp")):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(root, "include"), "-c", s, "-o",
                        os.path.join(d, "o.o")], check=True)
