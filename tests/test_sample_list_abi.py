"""Sample lists (sfw_samples_stage, sfw_score_samples): exported, declared in plain C99, ABI version unchanged, and the
argument checks that need no GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from social_force_window_planner_amd import planner
from social_force_window_planner_amd._abi import (EXPORTED_SYMBOLS, SFW_ERR_INVALID_ARG, SfwBest, SfwGoalArgs,
                                                   SfwRobotState)
from sfw_test_util import _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIST_SYMBOLS = ("sfw_samples_stage", "sfw_score_samples")


def test_list_symbols_declared_and_exported():
    declared = set(re.findall(r"\b(sfw_[a-z_0-9]+)\s*\(", _header()))
    assert set(LIST_SYMBOLS) <= declared and set(LIST_SYMBOLS) <= set(EXPORTED_SYMBOLS)
    L = planner.lib()
    assert all(hasattr(L, n) for n in LIST_SYMBOLS)
    assert all(planner.exported_symbols()[n] for n in LIST_SYMBOLS)


def test_abi_version_unchanged():
    assert planner.lib().sfw_abi_version() == 2
    assert re.search(r"#define SFW_ABI_VERSION 2\b", _header())


def test_null_handle_is_invalid_arg_without_gpu():
    L = planner.lib()
    rs, ga, best = SfwRobotState(0, 0, 0, 0, 0, 0), SfwGoalArgs(1, 1, 1, 1, 0), SfwBest()
    v = (C.c_double * 2)(0.1, 0.2)
    costs = (C.c_double * 2)()
    p = C.addressof(v)
    assert L.sfw_samples_stage(None, C.byref(rs), p, p, p, 2, C.byref(ga), 0) == SFW_ERR_INVALID_ARG
    assert L.sfw_samples_stage(None, C.byref(rs), p, None, p, 2, C.byref(ga), 0) == SFW_ERR_INVALID_ARG
    assert L.sfw_score_samples(None, C.byref(rs), p, p, p, 2, C.byref(ga), C.addressof(costs), C.byref(best)) == SFW_ERR_INVALID_ARG
    assert L.sfw_score_samples(None, None, None, None, None, 0, None, None, None) == SFW_ERR_INVALID_ARG


def test_header_compiles_as_c99_with_the_list_calls(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "l.c"
    src.write_text('#include "sfw_hip.h"\n#include <stddef.h>\n'
                   "int main(void) { sfw_robot_state rs = {0, 0, 0, 0, 0, 0}; sfw_goal_args ga = {1, 1, 1, 1, 0}; sfw_best b;\n"
                   "  double vx[2] = {0.1, 0.2}, vy[2] = {0, 0.1}, vth[2] = {0, 0.3}, c[2];\n"
                   "  return sfw_samples_stage(NULL, &rs, vx, vy, vth, 2, &ga, 0) + sfw_samples_stage(NULL, &rs, vx, NULL, vth, 2, &ga, 7) +\n"
                   "         sfw_score_samples(NULL, &rs, vx, vy, vth, 2, &ga, c, &b); }\n")
    r = subprocess.run([gcc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
