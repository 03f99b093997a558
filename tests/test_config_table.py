"""CPU-only: the range rules of the behaviour switches (csrc/tdr_config.cpp).  TUNING, CALLS and SPAN below were recorded
from the library as it was BEFORE the switches moved into one struct and one table — for every name of include/tdr.h's
knob list and every named tdr_config_* call, the default a query returns and the value in force after setting each
probe — and are replayed here: the table must answer as the scattered accessors did.  The two names removed with their
code paths ("su_wave_span", "su_lds_pad") answer -1 like any unknown name.  Also builds and runs
tests/cpp/config_override.cpp (the thread-local override scope of csrc/tdr_config.h, host code only)."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBES = [-5, -2, -1, 0, 1, 2, 3, 4, 5, 7, 8, 9, 33, 2047, 2048, 2049, 1 << 22, 1 << 30]
SPAN_PROBES = [-2.0, -1.0, 0.0, 0.5, 16.0, 40.0]
REMOVED = [-1] * len(PROBES)

# name: (default, the value returned after setting each of PROBES)
TUNING = {
    "score_waves": (131072, [131072, 131072, 131072, 131072, 1, 2, 3, 4, 5, 7, 8, 9, 33, 2047, 2048, 2049, 4194304, 1073741824]),
    "score_group": (0, [0, 0, 0, 0, 1, 2, 3, 4, 5, 7, 8, 9, 33, 2047, 2048, 2049, 4194304, 1073741824]),
    "su_group": (0, [0, 0, 0, 0, 1, 2, 3, 4, 5, 7, 8, 9, 33, 2047, 2048, 2049, 4194304, 1073741824]),
    "init_ahead": (1, [1, 1, 1, 1, 1, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3]),
    "batch_init_search": (0, [0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]),
    "prefix_head": (64, [64, 64, 64, 1, 1, 2, 3, 4, 5, 7, 8, 9, 33, 2047, 2048, 2048, 2048, 2048]),
    "ray_block_major": (1, [1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]),
    "ray_patch": (1, [1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]),
    "ray_borrow": (1, [1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]),
    "su_wave_span": (-1, REMOVED),
    "mt_stretches": (1, [1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]),
    "cart_seg_rows": (32, [32, 32, 32, 0, 0, 0, 0, 4, 4, 4, 8, 8, 32, 2044, 2048, 2048, 4194304, 1073741824]),
    "su_lds_pad": (-1, REMOVED),
    "su_tail_groups": (4, [4, 4, 4, 0, 1, 2, 3, 4, 5, 7, 8, 9, 33, 2047, 2048, 2049, 1048576, 1048576]),
    "su_tail_parts": (4, [4, 4, 4, 1, 1, 2, 2, 4, 4, 4, 8, 8, 8, 8, 8, 8, 8, 8]),
    "su_order_bucket": (1, [1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]),
    "init_device": (1, [1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]),
    "init_window_words": (2097152, [2097152, 2097152, 2097152, 2097152, 2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048, 4096, 4194304, 4194304]),
    "cart_init_chunk": (4096, [4096, 4096, 4096, 4096, 1, 2, 3, 4, 5, 7, 8, 9, 33, 2047, 2048, 2049, 4194304, 16777216]),
}
CALLS = {
    "tdr_config_compact": (1, [1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]),
    "tdr_config_shift_uniform": (1, [1, 1, 1, 0, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2]),
    "tdr_config_ray_split": (0, [0, 0, 0, 0, 1, 2, 3, 4, 5, 7, 8, 8, 8, 8, 8, 8, 8, 8]),
    "tdr_config_cart_skip": (1, [1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]),
    "tdr_config_init_mfma": (1, [1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]),
    "tdr_config_uw_waves": (1, [1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]),
    "tdr_config_prefix_small": (1, [1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]),
    "tdr_config_rec16_min_particles": (8192, [8192, 8192, 8192, 0, 1, 2, 3, 4, 5, 7, 8, 9, 33, 2047, 2048, 2049, 4194304, 1073741824]),
}
SPAN = (16.0, [16.0, 16.0, 0.0, 0.5, 16.0, 40.0])   # tdr_config_shift_uniform_span over SPAN_PROBES


@pytest.fixture(scope="module")
def lib():
    from top_down_renderer_amd import _lib, build
    build.build()
    return _lib.load()


def test_the_table_lists_what_the_header_lists():
    hdr = open(os.path.join(ROOT, "include", "tdr.h")).read()
    knob_list = hdr[hdr.index("tdr_config_tuning(name, value): value < 0 queries"):hdr.index("int64_t tdr_config_tuning(")]
    listed = set(re.findall(r'^ \*   "([a-z0-9_]+)"', knob_list, flags=re.M))
    assert listed == {n for n, (d, _) in TUNING.items() if d != -1}


@pytest.mark.parametrize("name", sorted(TUNING))
def test_tuning_rules_are_the_accessors_rules(lib, name):
    default, expected = TUNING[name]
    key = name.encode()
    try:
        assert lib.tdr_config_tuning(key, -1) == default
        for probe, want in zip(PROBES, expected):
            assert lib.tdr_config_tuning(key, probe) == want, f"{name}: set {probe}"
            assert lib.tdr_config_tuning(key, -1) == want, f"{name}: query after {probe}"
            if default >= 0:
                lib.tdr_config_tuning(key, default)
    finally:
        if default >= 0:
            assert lib.tdr_config_tuning(key, default) == default


@pytest.mark.parametrize("name", sorted(CALLS))
def test_named_calls_keep_their_rules(lib, name):
    default, expected = CALLS[name]
    call = getattr(lib, name)
    try:
        assert call(-1) == default
        for probe, want in zip(PROBES, expected):
            assert call(probe) == want, f"{name}({probe})"
            assert call(-1) == want
            call(default)
    finally:
        assert call(default) == default


def test_span_call_keeps_its_rules(lib):
    default, expected = SPAN
    try:
        assert lib.tdr_config_shift_uniform_span(-1.0) == default
        for probe, want in zip(SPAN_PROBES, expected):
            assert lib.tdr_config_shift_uniform_span(probe) == want, f"span({probe})"
            assert lib.tdr_config_shift_uniform_span(-1.0) == want
            lib.tdr_config_shift_uniform_span(-2.0)
    finally:
        assert lib.tdr_config_shift_uniform_span(-2.0) == default


def test_unknown_names_answer_minus_one(lib):
    assert lib.tdr_config_tuning(b"no_such_knob", 3) == -1
    assert lib.tdr_config_tuning(None, 3) == -1


def test_override_scope_is_thread_local(lib):
    """tests/cpp/config_override.cpp: TdrConfigScope against the process-wide struct, on two threads (host code only)."""
    pkg = os.path.join(ROOT, "top_down_renderer_amd")
    exe = os.path.join(tempfile.mkdtemp(prefix="tdr_config_"), "config_override")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(pkg, "csrc"), os.path.join(ROOT, "tests", "cpp", "config_override.cpp"), "-o", exe,
                    "-L", pkg, "-ltdr_hip", f"-Wl,-rpath,{pkg}"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == ["ok"], out.stdout
