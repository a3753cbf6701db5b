"""sfw_batch_* (many planners' control cycles in one launch): exported, declared in plain C99, and argument checks that
need no GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from social_force_window_planner_amd import planner
from social_force_window_planner_amd._abi import (EXPORTED_SYMBOLS, SFW_BATCH_MAX, SFW_ERR_INVALID_ARG, SFW_ERR_NO_DEVICE,
                                                   SFW_OK, SfwBatchDesc, default_params)
from sfw_test_util import _gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_SYMBOLS = ("sfw_batch_create", "sfw_batch_destroy", "sfw_batch_last_error", "sfw_batch_size", "sfw_batch_member",
                 "sfw_batch_launch", "sfw_batch_fetch", "sfw_batch_score_grid", "sfw_batch_describe", "sfw_batch_last_us")


def test_batch_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sfw_hip.h")).read()
    declared = set(re.findall(r"\b(sfw_[a-z_0-9]+)\s*\(", hdr))
    assert set(BATCH_SYMBOLS) <= declared and set(BATCH_SYMBOLS) <= set(EXPORTED_SYMBOLS)
    L = planner.lib()
    assert all(hasattr(L, n) for n in BATCH_SYMBOLS)
    assert re.search(r"#define SFW_BATCH_MAX 256\b", hdr) and SFW_BATCH_MAX == 256
    assert L.sfw_abi_version() == 2


def test_batch_header_is_plain_c99(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "b.c"
    src.write_text('#include "sfw_hip.h"\n#include <stddef.h>\n'
                   "int main(void) { sfw_batch b = NULL; sfw_batch_desc d; (void)d; return sfw_batch_size(b); }\n")
    r = subprocess.run([gcc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_batch_desc_layout():
    assert C.sizeof(SfwBatchDesc) == 32 and SfwBatchDesc.batch_blocks.offset == 16


def test_create_rejects_bad_arguments():
    L = planner.lib()
    p = default_params()
    b = C.c_void_p()
    for B in (0, -1, SFW_BATCH_MAX + 1):
        assert L.sfw_batch_create(C.byref(p), 0, B, C.byref(b)) == SFW_ERR_INVALID_ARG
        assert not b.value
    assert L.sfw_batch_create(C.byref(p), 0, 4, None) == SFW_ERR_INVALID_ARG
    assert L.sfw_batch_create(None, 0, 4, C.byref(b)) == SFW_ERR_INVALID_ARG
    bad = default_params(sim_granularity=0.0)
    assert L.sfw_batch_create(C.byref(bad), 0, 4, C.byref(b)) == SFW_ERR_INVALID_ARG


def test_null_batch_calls():
    L = planner.lib()
    d = SfwBatchDesc()
    us = C.c_double()
    assert L.sfw_batch_destroy(None) == SFW_OK
    assert L.sfw_batch_last_error(None) == b"null batch"
    assert L.sfw_batch_size(None) == 0
    assert L.sfw_batch_member(None, 0) is None
    assert L.sfw_batch_launch(None) == SFW_ERR_INVALID_ARG
    assert L.sfw_batch_fetch(None, None) == SFW_ERR_INVALID_ARG
    assert L.sfw_batch_score_grid(None, None, None, 0, None, 0, None, None) == SFW_ERR_INVALID_ARG
    assert L.sfw_batch_describe(None, C.byref(d)) == SFW_ERR_INVALID_ARG
    assert L.sfw_batch_last_us(None, 1, C.byref(us)) == SFW_ERR_INVALID_ARG


@pytest.mark.skipif(_gpu(), reason="a GPU is visible")
def test_batch_without_gpu_is_no_device():
    L = planner.lib()
    p = default_params()
    b = C.c_void_p()
    assert L.sfw_batch_create(C.byref(p), 0, 4, C.byref(b)) == SFW_ERR_NO_DEVICE
    assert not b.value
    with pytest.raises(planner.SfwError) as e:
        planner.BatchScorer(p, 0, 4)
    assert e.value.status == SFW_ERR_NO_DEVICE
