"""sfw_ensemble_* (one grid under several crowd hypotheses): exported, declared in plain C11, constants match the header,
argument checks that need no GPU, the aggregation kernels built into both translation units without scratch, and the
hypothesis builder."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from social_force_window_planner_amd import planner
from social_force_window_planner_amd import synthetic as syn
from social_force_window_planner_amd._abi import (EXPORTED_SYMBOLS, SFW_ENSEMBLE_MAX, SFW_ENSEMBLE_MAX_M, SFW_ENSEMBLE_MEAN,
                                                   SFW_ERR_INVALID_ARG, SFW_ERR_NO_DEVICE, SFW_OK, SfwBest, default_params)
from social_force_window_planner_amd.hypotheses import naive_goal_hypotheses
from kernel_listing import TUS, listing
from sfw_test_util import _gpu, _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENSEMBLE_SYMBOLS = ("sfw_ensemble_create", "sfw_ensemble_destroy", "sfw_ensemble_last_error", "sfw_ensemble_size",
                    "sfw_ensemble_member", "sfw_ensemble_set_params", "sfw_ensemble_set_costmap", "sfw_ensemble_set_footprint",
                    "sfw_ensemble_set_hypothesis", "sfw_ensemble_score_grid", "sfw_ensemble_aggregate", "sfw_ensemble_last_us")


def test_ensemble_symbols_declared_and_exported():
    declared = set(re.findall(r"\b(sfw_[a-z_0-9]+)\s*\(", _header()))
    assert set(ENSEMBLE_SYMBOLS) <= declared and set(ENSEMBLE_SYMBOLS) <= set(EXPORTED_SYMBOLS)
    L = planner.lib()
    assert all(hasattr(L, n) for n in ENSEMBLE_SYMBOLS)
    assert L.sfw_abi_version() == 2


def test_ensemble_constants_match_header():
    hdr = _header()
    for name, v in (("SFW_ENSEMBLE_MAX_M", SFW_ENSEMBLE_MAX_M), ("SFW_ENSEMBLE_MEAN", SFW_ENSEMBLE_MEAN),
                    ("SFW_ENSEMBLE_MAX", SFW_ENSEMBLE_MAX)):
        assert re.search(rf"#define {name} {v}\b", hdr), name
    assert (SFW_ENSEMBLE_MAX_M, SFW_ENSEMBLE_MEAN, SFW_ENSEMBLE_MAX) == (64, 0, 1)
    assert "typedef struct sfw_ensemble_s *sfw_ensemble;" in hdr


def test_ensemble_header_is_plain_c11(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "e.c"
    src.write_text('#include "sfw_hip.h"\n#include <stddef.h>\n'
                   "int main(void) {\n"
                   "  sfw_ensemble e = NULL; sfw_params p; sfw_best b; double c[45], us; int32_t r[45];\n"
                   "  sfw_robot_state rs = {0, 0, 0, 0, 0, 0}; sfw_goal_args ga = {1, 0, 1, 2, 0.5};\n"
                   "  const double lin[1] = {0.5}, ang[1] = {0.0}, prob[2] = {0.5, 0.5};\n"
                   "  sfw_params_default(&p);\n"
                   "  int rc = sfw_ensemble_create(&p, 0, SFW_ENSEMBLE_MAX_M, &e);\n"
                   "  rc |= sfw_ensemble_set_params(e, &p) | sfw_ensemble_set_footprint(e, NULL, 0);\n"
                   "  rc |= sfw_ensemble_set_costmap(e, NULL, 0, 0, 0.0, 0.0, 0.05) | sfw_ensemble_set_hypothesis(e, 0, NULL, 0, NULL, 0);\n"
                   "  rc |= sfw_ensemble_score_grid(e, &rs, lin, 1, ang, 1, &ga, SFW_ENSEMBLE_MEAN, prob, c, r, &b);\n"
                   "  rc |= sfw_ensemble_aggregate(e, SFW_ENSEMBLE_MAX, NULL, c, r, &b) | sfw_ensemble_last_us(e, 2, &us);\n"
                   "  sfw_handle h = sfw_ensemble_member(e, 0); (void)h; (void)sfw_ensemble_last_error(e);\n"
                   "  return rc + sfw_ensemble_size(e) + sfw_ensemble_destroy(e);\n"
                   "}\n")
    r = subprocess.run([gcc, "-std=c11", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_create_rejects_bad_m_without_device():
    L = planner.lib()
    p = default_params()
    e = C.c_void_p()
    for M in (0, -1, SFW_ENSEMBLE_MAX_M + 1, 1000):
        assert L.sfw_ensemble_create(C.byref(p), 0, M, C.byref(e)) == SFW_ERR_INVALID_ARG
        assert not e.value
    assert L.sfw_ensemble_create(C.byref(p), 0, 4, None) == SFW_ERR_INVALID_ARG
    assert L.sfw_ensemble_create(None, 0, 4, C.byref(e)) == SFW_ERR_INVALID_ARG
    bad = default_params(sim_granularity=0.0)
    assert L.sfw_ensemble_create(C.byref(bad), 0, 4, C.byref(e)) == SFW_ERR_INVALID_ARG
    with pytest.raises(planner.SfwError) as ex:
        planner.EnsembleScorer(p, 0, SFW_ENSEMBLE_MAX_M + 1)
    assert ex.value.status == SFW_ERR_INVALID_ARG


def test_null_ensemble_calls():
    L = planner.lib()
    p = default_params()
    us = C.c_double()
    best = SfwBest()
    assert L.sfw_ensemble_destroy(None) == SFW_OK
    assert L.sfw_ensemble_last_error(None) == b"null ensemble"
    assert L.sfw_ensemble_size(None) == 0
    assert L.sfw_ensemble_member(None, 0) is None
    assert L.sfw_ensemble_set_params(None, C.byref(p)) == SFW_ERR_INVALID_ARG
    assert L.sfw_ensemble_set_costmap(None, None, 0, 0, 0.0, 0.0, 0.05) == SFW_ERR_INVALID_ARG
    assert L.sfw_ensemble_set_footprint(None, None, 0) == SFW_ERR_INVALID_ARG
    assert L.sfw_ensemble_set_hypothesis(None, 0, None, 0, None, 0) == SFW_ERR_INVALID_ARG
    assert L.sfw_ensemble_score_grid(None, None, None, 0, None, 0, None, 0, None, None, None, C.byref(best)) == SFW_ERR_INVALID_ARG
    assert L.sfw_ensemble_aggregate(None, 0, None, None, None, C.byref(best)) == SFW_ERR_INVALID_ARG
    assert L.sfw_ensemble_last_us(None, 0, C.byref(us)) == SFW_ERR_INVALID_ARG


@pytest.mark.skipif(_gpu(), reason="a GPU is visible")
def test_ensemble_without_gpu_is_no_device():
    L = planner.lib()
    p = default_params()
    e = C.c_void_p()
    assert L.sfw_ensemble_create(C.byref(p), 0, 4, C.byref(e)) == SFW_ERR_NO_DEVICE
    assert not e.value
    with pytest.raises(planner.SfwError) as ex:
        planner.EnsembleScorer(p, 0, 4)
    assert ex.value.status == SFW_ERR_NO_DEVICE


@pytest.fixture(scope="module", params=TUS)
def resources(request):
    return request.param, listing(request.param).resources


@pytest.mark.parametrize("kernel", ["sfw_ensemble_stage1", "sfw_ensemble_stage2"])
def test_ensemble_kernels_without_scratch(resources, kernel):
    tu, res = resources
    names = [n for n in res if kernel in n]
    assert len(names) == 1, (tu, kernel, names)
    r = res[names[0]]
    assert r["scratch"] == 0, (tu, kernel, r)
    assert r["occupancy"] >= 4 and r["vgpr"] <= 128, (tu, kernel, r)


def _bits(x):
    return np.float64(x).view(np.uint64)


def test_naive_goal_hypotheses_reproduce_make_people():
    scene = syn.make_scene("ref5x9")  # make_people: goal = pos + 2.0 * vel
    (h,) = naive_goal_hypotheses(scene.agents, (2.0,))
    assert len(h) == len(scene.agents)
    for a, b in zip(scene.agents, h):
        assert bytes(a) == bytes(b)
    assert h[1].goal_x == scene.agents[1].x + 2.0 * scene.agents[1].vx  # (a copy, not the input array)
    h[1].goal_x = 99.0
    assert scene.agents[1].goal_x != 99.0


def test_naive_goal_hypotheses_rotation():
    scene = syn.make_scene(syn.WORKLOADS["cfg2"])
    times, offsets = (1.0, 3.0), (0.0, 0.4, -0.4)
    hyps = naive_goal_hypotheses(scene.agents, times, offsets)
    assert len(hyps) == len(times) * len(offsets)
    for k, h in enumerate(hyps):
        t, d = times[k // len(offsets)], offsets[k % len(offsets)]
        assert bytes(h[0]) == bytes(scene.agents[0]), "the robot is copied unchanged"
        for a, b in zip(scene.agents[1:], h[1:]):
            assert (a.x, a.y, a.radius, a.goal_radius, a.desired_velocity, a.has_goal, a.id, a.group_id) == \
                   (b.x, b.y, b.radius, b.goal_radius, b.desired_velocity, b.has_goal, b.id, b.group_id)
            assert math.isclose(math.hypot(a.vx, a.vy), math.hypot(b.vx, b.vy), rel_tol=1e-14), "rotation keeps the speed"
            turn = math.atan2(a.vx * b.vy - a.vy * b.vx, a.vx * b.vx + a.vy * b.vy)
            assert abs(turn - d) < 1e-12
            if d == 0.0:
                assert _bits(a.vx) == _bits(b.vx) and _bits(a.vy) == _bits(b.vy)
            assert b.goal_x == b.x + t * b.vx and b.goal_y == b.y + t * b.vy


@pytest.mark.gpu
def test_ensemble_set_costmap_refuses_non_finite_geometry_and_oversized_maps():
    """sfw_ensemble_set_costmap applies sfw_set_costmap's checks (sfw_hip.h) and names the failure"""
    L = planner.lib()
    e = planner.EnsembleScorer(default_params(), 0, 3)
    cells = np.zeros((4, 4), dtype=np.uint8)
    nan, inf = float("nan"), float("inf")
    for ox, oy, res in ((nan, 0.0, 0.05), (0.0, inf, 0.05), (0.0, 0.0, inf), (0.0, 0.0, nan)):
        assert L.sfw_ensemble_set_costmap(e._e, cells.ctypes.data, 4, 4, ox, oy, res) == SFW_ERR_INVALID_ARG, (ox, oy, res)
        assert b"set_costmap" in L.sfw_ensemble_last_error(e._e)
    for sx, sy in (((1 << 21) + 1, 1), (1 << 16, 1 << 15)):
        assert L.sfw_ensemble_set_costmap(e._e, cells.ctypes.data, sx, sy, 0.0, 0.0, 0.05) == SFW_ERR_INVALID_ARG, (sx, sy)
    e.set_costmap(cells, 0.0, 0.0, 0.05)
    e.close()
