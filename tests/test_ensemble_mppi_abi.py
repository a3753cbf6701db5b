"""Chained MPPI under crowd hypotheses (sfw_ensemble_blend_control, sfw_ensemble_mppi_run): declared in the header, exported by
the library, usable from plain C99, refused without a GPU for a NULL ensemble, and bound in Python with the header's argument
lists."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from social_force_window_planner_amd import planner
from social_force_window_planner_amd._abi import (EXPORTED_SYMBOLS, SFW_ERR_INVALID_ARG, SfwBest, SfwBlendStat, SfwGoalArgs, SfwMppi,
                                                   SfwPerturb, SfwRobotState)
from sfw_test_util import _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sfw_ensemble_blend_control", "sfw_ensemble_mppi_run")


def test_symbols_declared_and_exported():
    declared = set(re.findall(r"\b(sfw_[a-z_0-9]+)\s*\(", _header()))
    exported = planner.exported_symbols()
    for s in SYMBOLS:
        assert s in declared and s in EXPORTED_SYMBOLS and hasattr(planner.lib(), s) and exported[s], s
    # additive: the version stays
    assert planner.lib().sfw_abi_version() == 2 and re.search(r"#define SFW_ABI_VERSION 2\b", _header())


def test_header_compiles_as_c99_with_both_calls(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "m.c"
    src.write_text('#include "sfw_hip.h"\n#include <stddef.h>\n'
                   "int main(void) { double nominal[2 * 3] = {0.3, 0, 0, 0.3, 0, 0.1}, bias[4], u[2 * 3], w[4], plans[3 * 2 * 3], costs[4];\n"
                   "  double lambda = 0.5, probs[2] = {0.25, 0.75};\n"
                   "  int32_t steps[2] = {0, 5}, rejected[4];\n"
                   "  sfw_perturb p = {7u, 0, {0.1, 0, 0.2}, {0, 0, -0.5}, {0.7, 0, 0.5}, SFW_PERTURB_NO_VY, 0};\n"
                   "  sfw_mppi m = {3, 0, 0.5, 0.25};\n"
                   "  sfw_robot_state rs = {0, 0, 0, 0, 0, 0};\n"
                   "  sfw_goal_args ga = {1, 1, 1, 2, 0};\n"
                   "  sfw_blend_stat stat[SFW_MPPI_MAX_ITER];\n"
                   "  sfw_best best;\n"
                   "  sfw_ensemble e = NULL;\n"
                   "  p.nominal = nominal;\n"
                   "  return sfw_ensemble_blend_control(e, &lambda, 1, 0.25, bias, stat, u, w) +\n"
                   "         sfw_ensemble_mppi_run(e, &rs, &p, 4, 2, steps, &ga, SFW_ENSEMBLE_MEAN, probs, &m, stat, plans, costs, rejected,\n"
                   "                               &best) +\n"
                   "         sfw_ensemble_mppi_run(e, &rs, &p, 4, 2, steps, &ga, SFW_ENSEMBLE_MAX, NULL, &m, stat, plans, NULL, NULL, NULL); }\n")
    r = subprocess.run([gcc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_ensemble_is_invalid_arg_without_gpu():
    L = planner.lib()
    out = (C.c_double * 12)()
    stat = (SfwBlendStat * 2)()
    assert L.sfw_ensemble_blend_control(None, C.addressof(out), 1, 0.5, None, stat, C.addressof(out), None) == SFW_ERR_INVALID_ARG
    assert L.sfw_ensemble_blend_control(None, None, 0, float("nan"), None, None, None, None) == SFW_ERR_INVALID_ARG
    rs, ga, p, m, best = SfwRobotState(), SfwGoalArgs(), SfwPerturb(), SfwMppi(2, 0, 0.5, 0.3), SfwBest()
    assert L.sfw_ensemble_mppi_run(None, C.byref(rs), C.byref(p), 4, 1, None, C.byref(ga), 0, None, C.byref(m), stat, C.addressof(out),
                                   None, None, C.byref(best)) == SFW_ERR_INVALID_ARG
    assert L.sfw_ensemble_mppi_run(None, None, None, 0, 0, None, None, 7, None, None, None, None, None, None, None) == SFW_ERR_INVALID_ARG


# ---- the Python argument lists against the header's ------------------------------------------------------------------------------------
def _c_params(name):
    """The parameter types of `name` as the header declares them, comments and parameter names dropped."""
    text = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, name
    out = []
    for part in m.group(1).split(","):
        words = part.replace("*", " * ").split()
        stars = words.count("*")
        base = [w for w in words if w not in ("*", "const")][:-1]  # (the last word is the parameter's name)
        out.append((" ".join(base), stars))
    return out


def _ctype_of(base, stars):
    if stars == 0:
        return {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "sfw_ensemble": C.c_void_p}[base]
    typed = {"sfw_robot_state": SfwRobotState, "sfw_perturb": SfwPerturb, "sfw_goal_args": SfwGoalArgs, "sfw_mppi": SfwMppi,
             "sfw_blend_stat": SfwBlendStat, "sfw_best": SfwBest}
    return C.POINTER(typed[base]) if base in typed else C.c_void_p  # (plain arrays travel as addresses)


@pytest.mark.parametrize("name", SYMBOLS)
def test_argtypes_match_the_header(name):
    want = [_ctype_of(*p) for p in _c_params(name)]
    got = list(getattr(planner.lib(), name).argtypes)
    assert len(want) == {"sfw_ensemble_blend_control": 8, "sfw_ensemble_mppi_run": 15}[name]
    assert got == want, (name, got, want)
