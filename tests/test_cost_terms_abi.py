"""Per-term costs and re-scoring (sfw_set_terms_capture, sfw_grid_rescore, sfw_grid_terms): exported, declared in plain C99,
the ctypes struct matches the header, argument checks that need no GPU, and the re-score kernels built into both
translation units without scratch."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from social_force_window_planner_amd import planner
from social_force_window_planner_amd._abi import (EXPORTED_SYMBOLS, SFW_ERR_INVALID_ARG, SFW_N_TERMS, SFW_RESCORE_MAX_K,
                                                   SFW_TERM_ANGLE, SFW_TERM_COSTMAP, SFW_TERM_DISTANCE, SFW_TERM_SOCIAL,
                                                   SFW_TERM_VEL, SfwBest, SfwWeights)
from kernel_listing import TUS, listing
from sfw_test_util import _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERM_SYMBOLS = ("sfw_set_terms_capture", "sfw_grid_rescore", "sfw_grid_terms")


def test_term_symbols_declared_and_exported():
    declared = set(re.findall(r"\b(sfw_[a-z_0-9]+)\s*\(", _header()))
    assert set(TERM_SYMBOLS) <= declared and set(TERM_SYMBOLS) <= set(EXPORTED_SYMBOLS)
    L = planner.lib()
    assert all(hasattr(L, n) for n in TERM_SYMBOLS)
    assert L.sfw_abi_version() == 2


def test_term_constants_match_header():
    hdr = _header()
    for name, v in (("SFW_TERM_VEL", SFW_TERM_VEL), ("SFW_TERM_DISTANCE", SFW_TERM_DISTANCE), ("SFW_TERM_ANGLE", SFW_TERM_ANGLE),
                    ("SFW_TERM_COSTMAP", SFW_TERM_COSTMAP), ("SFW_TERM_SOCIAL", SFW_TERM_SOCIAL), ("SFW_N_TERMS", SFW_N_TERMS),
                    ("SFW_RESCORE_MAX_K", SFW_RESCORE_MAX_K)):
        assert re.search(rf"#define {name} {v}\b", hdr), name
    assert (SFW_TERM_VEL, SFW_TERM_DISTANCE, SFW_TERM_ANGLE, SFW_TERM_COSTMAP, SFW_TERM_SOCIAL, SFW_N_TERMS) == (0, 1, 2, 3, 4, 5)


def test_weights_struct_matches_header(tmp_path):
    assert [f for f, _ in SfwWeights._fields_] == ["vel", "distance", "angle", "costmap", "social"]
    assert C.sizeof(SfwWeights) == 40 and SfwWeights.social.offset == 32
    m = re.search(r"typedef struct sfw_weights \{\s*double ([^;]*);", _header())
    assert m and [s.strip() for s in m.group(1).split(",")] == ["vel", "distance", "angle", "costmap", "social"]
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "w.c"
    src.write_text('#include "sfw_hip.h"\n#include <stddef.h>\n'
                   "_Static_assert(sizeof(sfw_weights) == 40, \"size\");\n"
                   "_Static_assert(offsetof(sfw_weights, costmap) == 24, \"costmap\");\n"
                   "int main(void) { sfw_weights w = {1, 2, 3, 4, 5}; sfw_best b; double t[5];\n"
                   "  return sfw_grid_rescore(NULL, &w, 1, &b, NULL) + sfw_grid_terms(NULL, 0, 1, t) + sfw_set_terms_capture(NULL, 1); }\n")
    r = subprocess.run([gcc, "-std=c11", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_handle_and_bad_arguments_without_gpu():
    L = planner.lib()
    w = (SfwWeights * 2)(SfwWeights(1, 1, 1, 1, 1), SfwWeights(1, float("nan"), 1, 1, 1))
    best = (SfwBest * 2)()
    terms = (C.c_double * 5)()
    assert L.sfw_set_terms_capture(None, 1) == SFW_ERR_INVALID_ARG
    assert L.sfw_grid_rescore(None, w, 1, best, None) == SFW_ERR_INVALID_ARG
    assert L.sfw_grid_rescore(None, w, 0, best, None) == SFW_ERR_INVALID_ARG
    assert L.sfw_grid_rescore(None, w, SFW_RESCORE_MAX_K + 1, best, None) == SFW_ERR_INVALID_ARG
    assert L.sfw_grid_rescore(None, w, 2, best, None) == SFW_ERR_INVALID_ARG  # non-finite weight
    assert L.sfw_grid_terms(None, 0, 1, terms) == SFW_ERR_INVALID_ARG


@pytest.fixture(scope="module", params=TUS)
def resources(request):
    return request.param, listing(request.param).resources


@pytest.mark.parametrize("kernel", ["sfw_rescore_stage1", "sfw_rescore_stage2"])
def test_rescore_kernels_without_scratch(resources, kernel):
    tu, res = resources
    names = [n for n in res if kernel in n]
    assert len(names) == 1, (tu, kernel, names)
    r = res[names[0]]
    assert r["scratch"] == 0, (tu, kernel, r)
    # stage 1 holds one running selection (10 VGPRs) per weight vector of its tile: at least two waves per SIMD
    assert r["occupancy"] >= 2 and r["vgpr"] <= 256, (tu, kernel, r)
