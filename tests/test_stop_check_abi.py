"""sfw_set_stop_check and its queries: declared, exported, callable from plain C11, refused on a NULL handle with the outputs
untouched; the three tail kernels built for gfx950 without scratch and within their register budgets; the K1a kernels' resource
figures as the build before the stop check had them (the tail forms the rollout's end state itself, so none of them changes).
No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from social_force_window_planner_amd import planner
from social_force_window_planner_amd._abi import (EXPORTED_SYMBOLS, SFW_ERR_INVALID_ARG, SFW_STOP_MAX_STEPS, SFW_STOP_NONE, SFW_STOP_NOT_RUN,
                                                  SFW_STOP_UNFINISHED, SfwStopCheck, SfwStopRec)
from kernel_listing import KERNELS_TU, listing, one, source
from sfw_test_util import _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STOP_SYMBOLS = ("sfw_set_stop_check", "sfw_get_stop_check", "sfw_grid_stop_info", "sfw_grid_stop_points", "sfw_ensemble_set_stop_check")


def test_stop_symbols_declared_and_exported():
    hdr = _header()
    declared = set(re.findall(r"\b(sfw_[a-z_0-9]+)\s*\(", hdr))
    assert set(STOP_SYMBOLS) <= declared and set(STOP_SYMBOLS) <= set(EXPORTED_SYMBOLS)
    L = planner.lib()
    assert all(hasattr(L, n) for n in STOP_SYMBOLS)
    assert C.sizeof(SfwStopCheck) == 32 and C.sizeof(SfwStopRec) == 8
    for name, value in (("SFW_STOP_MAX_STEPS", SFW_STOP_MAX_STEPS), ("SFW_STOP_NONE", SFW_STOP_NONE),
                        ("SFW_STOP_UNFINISHED", SFW_STOP_UNFINISHED), ("SFW_STOP_NOT_RUN", SFW_STOP_NOT_RUN)):
        m = re.search(rf"#define {name} \(?(-?\d+)\)?", hdr)
        assert m and int(m.group(1)) == value, name
    assert (SFW_STOP_MAX_STEPS, SFW_STOP_NONE, SFW_STOP_UNFINISHED, SFW_STOP_NOT_RUN) == (4096, -1, -2, -3)
    assert L.sfw_abi_version() == 2 and "#define SFW_ABI_VERSION 2" in hdr
    # the header says what the check does, where it departs from the reference's dead code, and that the one-launch kernel
    # does not carry it
    for phrase in ("mayIStop", ":734-735", "> 0.0", "max_steps ends the loop", "one_launch = 0"):
        assert phrase in hdr, phrase


def test_stop_header_is_plain_c11(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "s.c"
    src.write_text('#include "sfw_hip.h"\n#include <stddef.h>\n'
                   "_Static_assert(sizeof(sfw_stop_check) == 32, \"sfw_stop_check\");\n"
                   "_Static_assert(sizeof(sfw_stop_rec) == 8, \"sfw_stop_rec\");\n"
                   "int main(void) {\n"
                   "  sfw_handle h = NULL; sfw_ensemble e = NULL; sfw_stop_check c = {1.0, 1.0, 1.0, SFW_STOP_MAX_STEPS, 0}, got;\n"
                   "  sfw_stop_rec rec = {0, SFW_STOP_NOT_RUN}; int32_t on = 0, n = 0; double pts[3];\n"
                   "  int rc = sfw_set_stop_check(h, &c) | sfw_set_stop_check(h, NULL) | sfw_get_stop_check(h, &got, &on);\n"
                   "  rc |= sfw_grid_stop_info(h, 0, 1, &rec) | sfw_grid_stop_points(h, 0, 1, 1, pts, &n);\n"
                   "  rc |= sfw_ensemble_set_stop_check(e, &c);\n"
                   "  return rc + on + n + rec.steps + (rec.hit == SFW_STOP_NONE) + (rec.hit == SFW_STOP_UNFINISHED);\n"
                   "}\n")
    r = subprocess.run([gcc, "-std=c11", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_handle_is_refused_and_outputs_stay():
    L = planner.lib()
    c, on = SfwStopCheck(0.5, 0.25, 0.125, 17, 0), C.c_int32(7)
    assert L.sfw_set_stop_check(None, C.byref(c)) == SFW_ERR_INVALID_ARG
    assert L.sfw_set_stop_check(None, None) == SFW_ERR_INVALID_ARG
    assert L.sfw_get_stop_check(None, C.byref(c), C.byref(on)) == SFW_ERR_INVALID_ARG
    assert L.sfw_ensemble_set_stop_check(None, C.byref(c)) == SFW_ERR_INVALID_ARG
    assert L.sfw_ensemble_set_stop_check(None, None) == SFW_ERR_INVALID_ARG
    assert (c.dec_x, c.dec_y, c.dec_theta, c.max_steps, c.reserved, on.value) == (0.5, 0.25, 0.125, 17, 0, 7)
    rec = np.full((2, 2), 99, dtype=np.int32)
    assert L.sfw_grid_stop_info(None, 0, 2, rec.ctypes.data) == SFW_ERR_INVALID_ARG
    pts, n = np.full((2, 3, 3), 7.0), np.full(2, 99, dtype=np.int32)
    assert L.sfw_grid_stop_points(None, 0, 2, 3, pts.ctypes.data, n.ctypes.data) == SFW_ERR_INVALID_ARG
    assert np.all(rec == 99) and np.all(pts == 7.0) and np.all(n == 99)


@pytest.fixture(scope="module")
def resources():
    return listing(KERNELS_TU).resources


def test_tail_kernels_without_scratch_and_within_budget(resources):
    """tests/test_kernel_resources.py pins no figure for sfw_footprint_kernel, so the budgets are stated here.  The tail's
    footprint kernel is sfw_footprint_kernel's body behind another load: no more registers than that kernel of the same build.
    The pose kernel and the finish kernel run 256-thread blocks, one thread per sample: at most 96 VGPRs (five waves per SIMD,
    the K1a kernels' own class), no scratch, no LDS."""
    fp = max(one(resources, f"sfw_footprint_kernelILb{b}E")["vgpr"] for b in (0, 1))
    k = one(resources, "sfw_stop_footprint_kernel")
    assert k["scratch"] == 0 and k["lds"] == 0 and k["vgpr"] <= fp, (k, fp)
    for name in ("sfw_stop_tail_kernel", "sfw_stop_finish_kernel"):
        k = one(resources, name)
        assert k["scratch"] == 0 and k["lds"] == 0 and k["vgpr"] <= 96, (name, k)


# (VGPRs, scratch bytes per lane, LDS bytes per block) of the K1a kernels <grid>, <list>, <sequence> in the build before the stop check
K1A_BEFORE = {
    "sfw_rollout_kernelILb0ELb0E": (88, 0, 0), "sfw_rollout_kernelILb1ELb0E": (88, 0, 0), "sfw_rollout_kernelILb1ELb1E": (94, 0, 0),
    "sfw_rollout_team_kernelILb0ELb0E": (97, 0, 3968), "sfw_rollout_team_kernelILb1ELb0E": (96, 0, 3968),
    "sfw_rollout_team_kernelILb1ELb1E": (98, 0, 3968),
    "sfw_rollout_small_kernelILb0ELb0E": (68, 136, 43056), "sfw_rollout_small_kernelILb1ELb0E": (66, 136, 43056),
    "sfw_rollout_small_kernelILb1ELb1E": (66, 136, 43056),
}


def test_k1a_kernels_keep_their_resources(resources):
    for name, want in K1A_BEFORE.items():
        k = one(resources, name)
        assert (k["vgpr"], k["scratch"], k["lds"]) == want, (name, k, want)


def test_tail_sits_above_the_contraction_pragma():
    src = source()
    off, fast = src.index("#pragma clang fp contract(off)"), src.index("#pragma clang fp contract(fast)")
    for name in ("sfw_stop_tail_kernel(", "sfw_stop_footprint_kernel(", "sfw_stop_finish_kernel("):
        assert off < src.index(name) < fast, name
    body = src[src.index("sfw_stop_tail_kernel("):src.index("sfw_stop_finish_kernel(")]
    assert "atomicMin" in body and "fma" not in body
