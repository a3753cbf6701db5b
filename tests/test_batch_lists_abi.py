"""The list forms of sfw_batch_* and the list-fusion switches: declared in plain C99, exported, prototyped in _abi.py, and the
argument checks that need no GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from social_force_window_planner_amd import planner
from social_force_window_planner_amd._abi import (EXPORTED_SYMBOLS, SFW_ERR_INVALID_ARG, SFW_ERR_NO_DEVICE, SfwBatchDesc,
                                                   default_params)
from sfw_test_util import _gpu, _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sfw_batch_set_list_fusion", "sfw_batch_get_list_fusion", "sfw_batch_score_samples", "sfw_batch_score_sequences",
               "sfw_batch_score_perturbed", "sfw_ensemble_set_list_fusion", "sfw_ensemble_get_list_fusion", "sfw_ensemble_batch_desc")


def test_symbols_declared_prototyped_and_exported():
    declared = set(re.findall(r"\b(sfw_[a-z_0-9]+)\s*\(", _header()))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(EXPORTED_SYMBOLS)
    L = planner.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n) and getattr(L, n).argtypes is not None, n
    assert all(planner.exported_symbols().values())
    assert L.sfw_abi_version() == 2


def test_desc_layout_is_unchanged():
    assert C.sizeof(SfwBatchDesc) == 32 and SfwBatchDesc.batch_blocks.offset == 16
    assert re.search(r"int32_t members, one_launch_members, own_path_members, batch_launches;\s*int64_t batch_blocks;\s*"
                     r"int32_t lds_bytes;\s*} sfw_batch_desc;", _header())


def test_header_is_plain_c99(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "b.c"
    src.write_text('#include "sfw_hip.h"\n#include <stddef.h>\n'
                   "int main(void) {\n  int32_t on = 7; sfw_batch_desc d; int64_t up = 0;\n"
                   "  int rc = sfw_batch_set_list_fusion(NULL, 1) + sfw_batch_get_list_fusion(NULL, &on);\n"
                   "  rc += sfw_batch_score_samples(NULL, NULL, NULL, NULL, NULL, 1, NULL, NULL);\n"
                   "  rc += sfw_batch_score_sequences(NULL, NULL, NULL, NULL, NULL, 1, 1, NULL, NULL, NULL);\n"
                   "  rc += sfw_batch_score_perturbed(NULL, NULL, NULL, 1, 1, NULL, NULL, NULL);\n"
                   "  rc += sfw_ensemble_set_list_fusion(NULL, 1) + sfw_ensemble_get_list_fusion(NULL, &on);\n"
                   "  rc += sfw_ensemble_batch_desc(NULL, &d, &up);\n  return rc == 8 * SFW_ERR_INVALID_ARG && on == 7 ? 0 : 1;\n}\n")
    exe = tmp_path / "b"
    lib_dir = os.path.join(ROOT, "social_force_window_planner_amd")
    r = subprocess.run([gcc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                        str(exe), "-L", lib_dir, "-lsfw_hip", f"-Wl,-rpath,{lib_dir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0


def test_null_handle_calls():
    L = planner.lib()
    on, d, up = C.c_int32(7), SfwBatchDesc(), C.c_int64()
    grid = L.sfw_batch_score_grid(None, None, None, 0, None, 0, None, None)
    assert grid == SFW_ERR_INVALID_ARG
    assert L.sfw_batch_score_samples(None, None, None, None, None, 1, None, None) == grid
    assert L.sfw_batch_score_sequences(None, None, None, None, None, 1, 1, None, None, None) == grid
    assert L.sfw_batch_score_perturbed(None, None, None, 1, 1, None, None, None) == grid
    assert L.sfw_batch_set_list_fusion(None, 1) == SFW_ERR_INVALID_ARG
    assert L.sfw_batch_get_list_fusion(None, C.byref(on)) == SFW_ERR_INVALID_ARG and on.value == 7
    assert L.sfw_ensemble_set_list_fusion(None, 1) == SFW_ERR_INVALID_ARG
    assert L.sfw_ensemble_get_list_fusion(None, C.byref(on)) == SFW_ERR_INVALID_ARG and on.value == 7
    assert L.sfw_ensemble_batch_desc(None, C.byref(d), C.byref(up)) == SFW_ERR_INVALID_ARG


@pytest.mark.skipif(_gpu(), reason="a GPU is visible")
def test_without_a_device_the_scorers_cannot_be_made():
    """(no batch, hence no handle the new calls could be given: the null-handle answers above are all there is without a GPU,
    as for sfw_batch_score_grid)"""
    p = default_params()
    for make in (lambda: planner.BatchScorer(p, 0, 3), lambda: planner.EnsembleScorer(p, 0, 3)):
        with pytest.raises(planner.SfwError) as e:
            make()
        assert e.value.status == SFW_ERR_NO_DEVICE


def test_python_surface():
    for name in ("set_list_fusion", "list_fusion", "stage_samples", "stage_sequences", "stage_perturbed", "score_samples",
                 "score_sequences", "score_perturbed"):
        assert callable(getattr(planner.BatchScorer, name)), name
    for name in ("set_list_fusion", "list_fusion", "batch_desc"):
        assert callable(getattr(planner.EnsembleScorer, name)), name
