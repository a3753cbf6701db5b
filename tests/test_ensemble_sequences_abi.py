"""sfw_ensemble_score_sequences / _score_perturbed / _blend (MPPI rollouts under several crowd hypotheses): declared, exported,
callable from plain C11, NULL handles refused, ABI version unchanged, and the list form of the aggregation kernel built
without scratch inside the register and occupancy bounds tests/test_ensemble_abi.py holds the grid form to."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from social_force_window_planner_amd import planner
from social_force_window_planner_amd._abi import EXPORTED_SYMBOLS, SFW_ERR_INVALID_ARG, SfwBest, SfwBlendStat
from kernel_listing import KERNELS_TU, listing
from sfw_test_util import _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sfw_ensemble_score_sequences", "sfw_ensemble_score_perturbed", "sfw_ensemble_blend")
LIST_KERNEL = "sfw_ens_list_first"


def test_symbols_declared_exported_and_listed():
    declared = set(re.findall(r"\b(sfw_[a-z_0-9]+)\s*\(", _header()))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(EXPORTED_SYMBOLS)
    L = planner.lib()
    assert all(hasattr(L, n) for n in NEW_SYMBOLS)
    assert all(planner.exported_symbols()[n] for n in NEW_SYMBOLS)


def test_abi_version_stays_2():
    assert planner.lib().sfw_abi_version() == 2
    assert re.search(r"#define SFW_ABI_VERSION 2\b", _header())


def test_header_is_plain_c11(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "es.c"
    src.write_text('#include "sfw_hip.h"\n#include <stddef.h>\n'
                   "int main(void) {\n"
                   "  sfw_ensemble e = NULL; sfw_best b; double c[4], u[2 * 2 * 3], w[2 * 4]; int32_t r[4];\n"
                   "  sfw_robot_state rs = {0, 0, 0, 0, 0, 0}; sfw_goal_args ga = {1, 0, 1, 2, 0.5};\n"
                   "  const double vx[8] = {0.5, 0.4, 0.3, 0.2, 0.5, 0.4, 0.3, 0.2}, vth[8] = {0}, prob[2] = {0.5, 0.5};\n"
                   "  const double nominal[6] = {0.4, 0.0, 0.0, 0.3, 0.0, 0.1}, lambda[2] = {0.5, 2.0}, bias[4] = {0, 0, 0, 0};\n"
                   "  const int32_t steps[2] = {0, 10};\n"
                   "  sfw_perturb p = {7u, nominal, {0.1, 0.0, 0.2}, {0.0, 0.0, -0.5}, {0.7, 0.0, 0.5}, SFW_PERTURB_NO_VY, 0};\n"
                   "  sfw_blend_stat st[2];\n"
                   "  int rc = sfw_ensemble_score_sequences(e, &rs, vx, NULL, vth, 4, 2, steps, &ga, SFW_ENSEMBLE_MEAN, prob, c, r, &b);\n"
                   "  rc |= sfw_ensemble_score_perturbed(e, &rs, &p, 4, 2, steps, &ga, SFW_ENSEMBLE_MAX, NULL, c, r, &b);\n"
                   "  rc |= sfw_ensemble_blend(e, lambda, 2, bias, st, u, w);\n"
                   "  return rc;\n"
                   "}\n")
    r = subprocess.run([gcc, "-std=c11", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_ensemble_calls():
    L = planner.lib()
    best = SfwBest()
    stat = (SfwBlendStat * 1)()
    lam, u = (C.c_double * 1)(1.0), (C.c_double * 3)()
    assert L.sfw_ensemble_score_sequences(None, None, None, None, None, 0, 0, None, None, 0, None, None, None,
                                          C.byref(best)) == SFW_ERR_INVALID_ARG
    assert L.sfw_ensemble_score_perturbed(None, None, None, 0, 0, None, None, 0, None, None, None, C.byref(best)) == SFW_ERR_INVALID_ARG
    assert L.sfw_ensemble_blend(None, lam, 1, None, stat, u, None) == SFW_ERR_INVALID_ARG
    assert L.sfw_ensemble_blend(None, None, 0, None, None, None, None) == SFW_ERR_INVALID_ARG


def test_list_kernel_without_scratch():
    """Costs and terms are doubles in every precision mode: the kernel exists in the default translation unit only."""
    res = listing(KERNELS_TU).resources
    names = [n for n in res if LIST_KERNEL in n]
    assert len(names) == 1, names
    assert "sfw_ensemble_stage1" not in names[0]  # (the grid form stays the one symbol of that name)
    r = res[names[0]]
    assert r["scratch"] == 0, r
    assert r["occupancy"] >= 4 and r["vgpr"] <= 128, r
