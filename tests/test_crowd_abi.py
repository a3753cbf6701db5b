"""The predicted crowd (sfw_score_one_crowd, sfw_grid_crowd): exported, declared in plain C99, ABI version unchanged, and the
argument checks that need no GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from social_force_window_planner_amd import planner
from social_force_window_planner_amd._abi import EXPORTED_SYMBOLS, SFW_ERR_INVALID_ARG, SfwGoalArgs, SfwRobotState
from sfw_test_util import _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROWD_SYMBOLS = ("sfw_score_one_crowd", "sfw_grid_crowd")


def test_crowd_symbols_declared_and_exported():
    declared = set(re.findall(r"\b(sfw_[a-z_0-9]+)\s*\(", _header()))
    assert set(CROWD_SYMBOLS) <= declared and set(CROWD_SYMBOLS) <= set(EXPORTED_SYMBOLS)
    L = planner.lib()
    assert all(hasattr(L, n) for n in CROWD_SYMBOLS)
    assert all(planner.exported_symbols()[n] for n in CROWD_SYMBOLS)


def test_abi_version_unchanged():
    assert planner.lib().sfw_abi_version() == 2
    assert re.search(r"#define SFW_ABI_VERSION 2\b", _header())


def test_null_handle_is_invalid_arg_without_gpu():
    L = planner.lib()
    rs, ga = SfwRobotState(0, 0, 0, 0, 0, 0), SfwGoalArgs(1, 1, 1, 1, 0)
    cost, n = C.c_double(), C.c_int32(-7)
    state, work, hg = (C.c_double * 8)(), (C.c_double * 2)(), (C.c_int32 * 2)()
    assert L.sfw_score_one_crowd(None, C.byref(rs), 0.5, 0.0, 0.2, C.byref(ga), C.byref(cost), C.addressof(state),
                                 C.addressof(work), C.addressof(hg), 2, 1, C.byref(n)) == SFW_ERR_INVALID_ARG
    assert L.sfw_score_one_crowd(None, None, 0.0, 0.0, 0.0, None, None, None, None, None, 0, 0, None) == SFW_ERR_INVALID_ARG
    assert L.sfw_grid_crowd(None, 0, C.byref(cost), C.addressof(state), C.addressof(work), C.addressof(hg), 2, 1,
                            C.byref(n)) == SFW_ERR_INVALID_ARG
    assert L.sfw_grid_crowd(None, 0, None, None, None, None, 0, 0, None) == SFW_ERR_INVALID_ARG
    assert n.value == -7  # nothing written


def test_header_compiles_as_c99_with_the_crowd_calls(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "c.c"
    src.write_text('#include "sfw_hip.h"\n#include <stddef.h>\n'
                   "int main(void) { sfw_robot_state rs = {0, 0, 0, 0, 0, 0}; sfw_goal_args ga = {1, 1, 1, 1, 0};\n"
                   "  double cost, state[2 * 3 * 4], work[2 * 3]; int32_t hg[2 * 3], n;\n"
                   "  return sfw_score_one_crowd(NULL, &rs, 0.5, 0.0, 0.2, &ga, &cost, state, work, hg, 3, 2, &n) +\n"
                   "         sfw_score_one_crowd(NULL, &rs, 0.5, 0.0, 0.2, &ga, &cost, state, NULL, NULL, 3, 2, &n) +\n"
                   "         sfw_grid_crowd(NULL, 7, &cost, state, work, hg, 3, 2, &n) + sfw_grid_crowd(NULL, 7, NULL, state, NULL, NULL, 3, 2, &n); }\n")
    r = subprocess.run([gcc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
