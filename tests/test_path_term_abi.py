"""sfw_set_path and its companions: declared, exported, callable from plain C11 with the struct layout _abi.py states, refused on
a NULL handle with the outputs untouched; the header states the definition; the three new kernels built for gfx950 without
scratch or LDS and within their register budget, under the rollout's no-contraction pragma.  No GPU (the refusals that need a
handle are in tests/test_path_term_gpu.py::test_state_and_errors)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from social_force_window_planner_amd import planner
from social_force_window_planner_amd._abi import (EXPORTED_SYMBOLS, SFW_ERR_INVALID_ARG, SFW_PATH_MAX_COORD, SFW_PATH_MAX_POINTS, SFW_N_TERMS,
                                                  SfwBest, SfwPath, SfwWeights)
from kernel_listing import KERNELS_TU, listing, one, source
from sfw_test_util import _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "social_force_window_planner_amd", "csrc")
PATH_SYMBOLS = ("sfw_set_path", "sfw_get_path", "sfw_grid_path_term", "sfw_grid_rescore_path", "sfw_ensemble_set_path")


def test_path_symbols_declared_and_exported():
    hdr = _header()
    declared = set(re.findall(r"\b(sfw_[a-z_0-9]+)\s*\(", hdr))
    assert set(PATH_SYMBOLS) <= declared and set(PATH_SYMBOLS) <= set(EXPORTED_SYMBOLS)
    L = planner.lib()
    assert all(hasattr(L, n) for n in PATH_SYMBOLS)
    assert C.sizeof(SfwPath) == 24
    assert (SfwPath.xy.offset, SfwPath.n_points.offset, SfwPath.reserved.offset, SfwPath.weight.offset) == (0, 8, 12, 16)
    m = re.search(r"#define SFW_PATH_MAX_POINTS (\d+)", hdr)
    assert m and int(m.group(1)) == SFW_PATH_MAX_POINTS == 1024
    m = re.search(r"#define SFW_PATH_MAX_COORD (\S+)", hdr)
    assert m and float(m.group(1)) == SFW_PATH_MAX_COORD == 1e7
    # the term is a sixth one beside the captured five, and the ABI version stays
    assert L.sfw_abi_version() == 2 and "#define SFW_ABI_VERSION 2" in hdr and SFW_N_TERMS == 5 and C.sizeof(SfwWeights) == 40
    # the header states the definition, operation by operation, and what the setting reaches
    for phrase in ("u  = (rx*ex + ry*ey) * inv", "t  = u < 0 ? 0 : (u > 1 ? 1 : u)", "qx = rx - t*ex;  qy = ry - t*ey",
                   "d  = qx*qx + qy*qy", "inv = len2 > 0 ? 1.0/len2 : 0.0", "`d < m ? d : m` from m = +inf",
                   "p = (((D_0 + D_1) + D_2) + ... + D_{S-1}) / S", "cost5 + path_weight * p", "one_launch = 0", "own_path_members",
                   "read by the next stage", "taken from\n * member 0", "sfw_ensemble_member"):
        assert phrase in hdr, phrase


def test_path_header_is_plain_c11(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "p.c"
    src.write_text('#include "sfw_hip.h"\n#include <stddef.h>\n'
                   "_Static_assert(sizeof(sfw_path) == 24, \"sfw_path\");\n"
                   "_Static_assert(offsetof(sfw_path, xy) == 0 && offsetof(sfw_path, n_points) == 8, \"sfw_path\");\n"
                   "_Static_assert(offsetof(sfw_path, reserved) == 12 && offsetof(sfw_path, weight) == 16, \"sfw_path\");\n"
                   "int main(void) {\n"
                   "  sfw_handle h = NULL; sfw_ensemble e = NULL; double xy[4] = {0, 0, 1, 1}, out[4], w = 0, pw[2] = {0, -1};\n"
                   "  sfw_path p = {xy, 2, 0, 1.5}; int32_t n = 0, on = 0; sfw_weights ws = {1, 1, 1, 1, 1}; sfw_best b[2];\n"
                   "  int rc = sfw_set_path(h, &p) | sfw_set_path(h, NULL) | sfw_get_path(h, out, 2, &n, &w, &on);\n"
                   "  rc |= sfw_grid_path_term(h, 0, 1, out) | sfw_grid_rescore_path(h, &ws, pw, 2, b, NULL);\n"
                   "  rc |= sfw_ensemble_set_path(e, &p) | (SFW_PATH_MAX_POINTS != 1024) | (SFW_PATH_MAX_COORD != 1e7);\n"
                   "  return rc + n + on;\n"
                   "}\n")
    r = subprocess.run([gcc, "-std=c11", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_handle_is_refused_and_outputs_stay():
    L = planner.lib()
    xy = np.array([[0.0, 0.0], [1.0, 1.0]])
    p = SfwPath(xy.ctypes.data_as(C.POINTER(C.c_double)), 2, 0, 1.5)
    assert L.sfw_set_path(None, C.byref(p)) == SFW_ERR_INVALID_ARG
    assert L.sfw_set_path(None, None) == SFW_ERR_INVALID_ARG
    assert L.sfw_ensemble_set_path(None, C.byref(p)) == SFW_ERR_INVALID_ARG
    assert L.sfw_ensemble_set_path(None, None) == SFW_ERR_INVALID_ARG
    out, n, w, on = np.full((2, 2), 7.0), C.c_int32(9), C.c_double(3.5), C.c_int32(5)
    assert L.sfw_get_path(None, out.ctypes.data, 2, C.byref(n), C.byref(w), C.byref(on)) == SFW_ERR_INVALID_ARG
    assert np.all(out == 7.0) and (n.value, w.value, on.value) == (9, 3.5, 5)
    term = np.full(3, 7.0)
    assert L.sfw_grid_path_term(None, 0, 3, term.ctypes.data) == SFW_ERR_INVALID_ARG and np.all(term == 7.0)
    ws, pw, best, costs = SfwWeights(1, 1, 1, 1, 1), np.array([0.0, -1.0]), (SfwBest * 2)(), np.full(4, 7.0)
    assert L.sfw_grid_rescore_path(None, C.byref(ws), pw.ctypes.data, 2, best, costs.ctypes.data) == SFW_ERR_INVALID_ARG
    assert np.all(costs == 7.0)
    assert (p.n_points, p.reserved, p.weight) == (2, 0, 1.5)


@pytest.fixture(scope="module")
def resources():
    return listing(KERNELS_TU).resources


def test_path_kernels_without_scratch_and_within_budget(resources):
    """256-thread blocks, one thread per (step, sample) or per sample, a handful of doubles live: at most 64 VGPRs (eight waves per
    SIMD — the kernels wait on memory, the distance kernel on its scalar loads), no scratch, no LDS.  The re-score and ensemble
    kernels that took the nullable term pointer keep the budgets their own tests state."""
    for name in ("sfw_path_fill_kernel", "sfw_path_dist_kernel", "sfw_path_scan_kernel", "sfw_path_add_kernel"):
        k = one(resources, name)
        assert k["scratch"] == 0 and k["lds"] == 0 and k["vgpr"] <= 64 and k["occupancy"] >= 8, (name, k)
    # the existing resource tests find kernels by substring: no existing kernel's name occurs in a new one's
    for old in ("sfw_footprint_kernel", "sfw_costmap_scan", "sfw_stop_", "sfw_rescore_stage", "sfw_ensemble_stage", "sfw_ens_"):
        assert not [n for n in resources if "sfw_path_" in n and old in n]


def test_path_kernels_sit_under_the_no_contraction_pragma():
    src = source()
    off, fast = src.index("#pragma clang fp contract(off)"), src.index("#pragma clang fp contract(fast)")
    for name in ("sfw_path_fill_kernel(", "sfw_path_dist_kernel(", "sfw_path_scan_kernel(", "sfw_path_add_kernel("):
        assert off < src.index(name) < fast, name
    body = src[src.index("sfw_path_dist_kernel("):src.index("sfw_path_add_kernel(")]
    # no fused multiply-add, and the one atomic is the integer minimum on the bit pattern (exact in any order): no
    # floating-point atomic
    assert "fma" not in body and body.count("atomic") == 1 and "atomicMin(reinterpret_cast<unsigned long long *>" in body
    dev = open(os.path.join(CSRC, "sfw_device.h")).read()
    add = dev[dev.index("sfw_cost_add_path("):]
    assert "#pragma clang fp contract(off)" in add[:200]
