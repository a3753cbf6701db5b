"""The shared-prefix tree over its WORK ITEMS (row classes(p) x column classes(p - 1) for a level ending at step p: the column
axis lags by one step, include/sfw_hip.h sfw_plan_shared_prefix_items) must not show in the results: costs, sentinels, selection,
contact steps and the captured cost terms are np.array_equal to the same scene under SFW_PREFIX=0, in every organisation of a K2
wave, for one-step levels, a level ending at S - 1, two steps in all, chunked tables, groups and laser points, single precision,
contacts inside a level, at a level's last step and at a child's first step, the host-evaluated pinned-rest table and a grid cut
into two ranks' row blocks.  The kernels are the parent's: their resource figures are pinned at the end."""
import dataclasses
import math
import os

import numpy as np
import pytest

from kernel_listing import TUS, listing, one
from sfw_test_util import _workload_params
from social_force_window_planner_amd import synthetic as syn
from social_force_window_planner_amd._abi import SFW_MULTI_HOST_REDUCE, SFW_ORG_FLAT, SFW_ORG_REGISTER_1, SFW_PRECISION_F32, default_params

gpu = pytest.mark.gpu


def _run(hip_mod, scene, params, prefix, budget_mb=None, rs=None):
    """One grid call on a fresh handle created under SFW_PREFIX=<prefix>: everything a caller can read back"""
    env = {"SFW_PREFIX": str(prefix), "SFW_TABLE_BUDGET_MB": None if budget_mb is None else str(budget_mb)}
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        g = hip_mod.HipScorer(params)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    g.load_scene(scene)
    g.set_terms_capture(True)
    costs, best = g.score_grid(rs or scene.robot_state, scene.linvels, scene.angvels, scene.goal_args)
    out = {"costs": costs, "best": best, "terms": g.cost_terms(), "plan": g.plan_info()}
    _, n = g.grid_points_batch(0, len(costs), scene.workload.n_steps)
    out["coll_step"] = np.where(costs == -1.0, n - 1, -1)  # a Trajectory ends with the pose of the step that met a pedestrian
    g.close()
    return out


def _assert_same(ref, got, what):
    for k in ("costs", "terms", "coll_step"):
        assert np.array_equal(ref[k], got[k], equal_nan=True), (what, k)
    assert np.array_equal(ref["costs"] < 0, got["costs"] < 0) and ref["best"] == got["best"], what


def _check(hip_mod, scene, params, prefixes, rs=None, budget_mb=None, levels=None):
    ref = _run(hip_mod, scene, params, 0, rs=rs)
    assert ref["plan"]["levels"] == 0 and (ref["costs"] >= 0).sum() > 0
    for prefix in prefixes:
        got = _run(hip_mod, scene, params, prefix, budget_mb=budget_mb, rs=rs)
        if prefix != -1:  # (the automatic plan may find nothing worth sharing)
            assert got["plan"]["levels"] == (levels if levels is not None else len(str(prefix).split(","))), prefix
        _assert_same(ref, got, prefix)
    return ref


def _scene(name, nv, nw, people, **kw):
    return syn.make_scene(dataclasses.replace(syn.WORKLOADS[name], nv=nv, nw=nw, n_people=people, **kw))


LEVELS = (-1, "1", "1,2,3", "2,4,9")  # automatic; one level of one step; one-step levels; the usual kind


@gpu
def test_register_form(hip_mod):
    """72 x 72 samples, 9 people, cfg2's parameters: six samples per register-form wave"""
    scene = _scene("cfg2", 72, 72, 9)
    S = scene.workload.n_steps
    ref = _check(hip_mod, scene, _workload_params(scene.workload), LEVELS + (str(S - 1),))
    assert ref["plan"]["organisation"] == SFW_ORG_REGISTER_1


@gpu
def test_flat_form(hip_mod):
    """64 x 64 samples, 50 people: one sample per wave, 64-double planes"""
    scene = _scene("target", 64, 64, 50)
    S = scene.workload.n_steps
    ref = _check(hip_mod, scene, _workload_params(scene.workload), LEVELS + (str(S - 1),))
    assert ref["plan"]["organisation"] == SFW_ORG_FLAT


@gpu
@pytest.mark.parametrize("nv,nw,people", [(72, 72, 21), (80, 80, 20)])
def test_mixed_launch(hip_mod, nv, nw, people):
    """72 x 72 with 21 people; and 80 x 80 with 20 (21 agents, three samples per register-form wave: 6400 samples are two waves per
    SIMD and 256 samples over), where the launch over the samples is the mixed kernel by the launch plan's own rule"""
    scene = _scene("cfg2", nv, nw, people)
    ref = _check(hip_mod, scene, _workload_params(scene.workload), (-1, "1", "2,4,9"))
    if people == 20:
        assert ref["plan"]["organisation"] == SFW_ORG_REGISTER_1 and ref["plan"]["flat_samples"] > 0


@gpu
def test_two_steps_in_all(hip_mod):
    scene = _scene("cfg2", 72, 72, 9, sim_time=0.05)
    assert scene.workload.n_steps == 2
    _check(hip_mod, scene, _workload_params(scene.workload), ("1",), levels=1)


@gpu
def test_chunks_of_whole_rows(hip_mod):
    """a 1 MiB table budget: several chunks, each with its own row tables over the one lagged column axis"""
    scene = _scene("cfg2", 72, 72, 9)
    ref = _run(hip_mod, scene, _workload_params(scene.workload), 0)
    for prefix in (-1, "1", "2,4,9"):
        got = _run(hip_mod, scene, _workload_params(scene.workload), prefix, budget_mb=1)
        assert got["plan"]["chunks"] > 1 and (prefix == -1 or got["plan"]["levels"] > 0)
        _assert_same(ref, got, prefix)


@gpu
@pytest.mark.parametrize("precision", [None, SFW_PRECISION_F32])
def test_group_laser_points_and_single_precision(hip_mod, precision):
    scene = _scene("cfg2", 72, 72, 12, n_obstacles=8, seed=19)
    for i in (2, 3, 4):
        scene.agents[i].group_id = 7
    kw = {} if precision is None else {"precision": precision}
    _check(hip_mod, scene, _workload_params(scene.workload, **kw), (-1, "1", "1,2,3", "2,4,9"))


@gpu
@pytest.mark.parametrize("target,where", [(6, "inside a level"), (8, "a level's last step"), (9, "a child's first step")])
def test_contacts(hip_mod, oracle_mod, target, where):
    """Levels [0,4) [4,9) [9,14): a person crosses the robot's way 0.4 m ahead of it at 1 m/s, from where the CPU oracle's
    Trajectory of the fastest straight sample ends at step `target` — its class dies there, the members inherit the verdict and
    the step; the slower samples (two thirds of the rows, a few centimetres behind by then) pass or touch later"""
    scene = _scene("cfg2", 72, 72, 9, n_discs=0)
    w = scene.workload
    lin, ang = scene.linvels, scene.angvels
    iv, iw = len(lin) - 1, int(np.argmin(np.abs(ang)))
    o = oracle_mod.OracleScorer(_workload_params(w))
    a = scene.agents[1]
    a.x = a.goal_x = scene.robot_state[0] + 0.4
    a.vx, a.vy, a.goal_y = 0.0, -1.0, scene.robot_state[1] - 3.0
    found = None
    for mm in range(100, 500):  # where the person starts, to the robot's left, 1 mm apart
        a.y = scene.robot_state[1] + mm / 1000.0
        o.load_scene(scene)
        cost, pts = o.score_one(scene.robot_state, float(lin[iv]), 0.0, float(ang[iw]), scene.goal_args)
        if cost == -1.0 and len(pts) - 1 == target:
            found = mm
            break
    assert found is not None, where
    ref = _check(hip_mod, scene, _workload_params(w), ("4,9,14", -1))
    t = iv * len(ang) + iw
    assert ref["coll_step"][t] == target  # the case really occurs on the device too
    assert len(set(ref["coll_step"][ref["coll_step"] >= 0])) > 1  # ... among contacts at other steps


@gpu
def test_pinned_rest_table(hip_mod):
    """The stopped robot among people that can never move of test_parity_holes_gpu.py (its pin_rest set, the 64 x 66 grid): the
    linvel = 0 row takes the host-evaluated table's lateral force and Wp corrections at every step, inside the levels too"""
    import test_parity_holes_gpu as holes

    scene = _scene("cfg2", 64, 66, 12, seed=735)
    ag, rs = scene.agents, scene.robot_state
    rs = (rs[0], rs[1], rs[2], 0.0, 0.0, 0.0)
    ag[0].vx = ag[0].vy = 0.0
    rng = np.random.default_rng(99)
    for i in (2, 5, 6, 8, 11):
        for _ in range(100000):
            r, a = rng.uniform(1.2, 2.5), rng.uniform(-math.pi, math.pi)
            x, y = rs[0] + r * math.cos(a), rs[1] + r * math.sin(a)
            sg = (holes._noise_sign(rs[0], rs[1], x, y), holes._noise_sign(x, y, rs[0], rs[1]))
            if sg != (0, 0) and all(math.hypot(x - ag[j].x, y - ag[j].y) > 0.8 for j in range(1, len(ag)) if j != i):
                break
        ag[i].x, ag[i].y = x, y
        if i != 8:
            holes._stand(ag[i])
        ag[i].desired_velocity = 0.0
    assert scene.linvels[0] == 0.0
    ref = _check(hip_mod, scene, default_params(), ("4,9", "1", -1), rs=rs)
    assert (ref["costs"][:66] >= 0).sum() >= 4


@gpu
def test_two_ranks_row_blocks(hip_mod, monkeypatch):
    """128 x 64 samples cut into two ranks' row blocks (each plans its own tree over the lent column axis) against the whole grid"""
    scene = _scene("cfg2", 128, 64, 9)
    p = _workload_params(scene.workload)
    ref = _run(hip_mod, scene, p, 0)
    for prefix in (None, "1", "2,4,9"):
        if prefix is None:
            monkeypatch.delenv("SFW_PREFIX", raising=False)
        else:
            monkeypatch.setenv("SFW_PREFIX", prefix)
        m = hip_mod.MultiScorer(p, devices=(0, 0), exchange=SFW_MULTI_HOST_REDUCE)
        m.load_scene(scene)
        costs, best = m.score_grid(scene.robot_state, scene.linvels, scene.angvels, scene.goal_args)
        assert prefix is None or all(hip_mod.plan_info_of_rank(m, r)["levels"] > 0 for r in range(2))
        m.close()
        assert np.array_equal(ref["costs"], costs) and ref["best"] == best, prefix


# ---- the kernels are the parent's (no GPU needed: the compiler's resource remarks) ------------------------------------------
# (VGPRs, scratch bytes per lane, waves per SIMD) in both builds of the kernel units
PARENT_FIGURES = {
    "sfw_social_kernelIdLi1ELb0E": (77, 0, 6),
    "sfw_social_kernelIdLi1ELb1E": (89, 0, 5),
    "sfw_social_kernelIdLi2ELb0E": (91, 0, 5),
    "sfw_social_kernel_flatIdLb0ELi64ELb0E": (80, 0, 6),
    "sfw_social_kernel_flatIdLb0ELi64ELb1E": (96, 24, 5),
    "sfw_social_kernel_flatIdLb0ELi128ELb0E": (76, 0, 6),
    "sfw_social_kernel_flatIdLb0ELi256ELb0E": (76, 0, 6),
    "sfw_social_kernel_flatIdLb1ELi64ELb1E": (122, 0, 4),
    "sfw_social_kernel_mixedId": (80, 12, 6),
    "sfw_cycle_kernelIdLb0ELb0E": (85, 136, 5),
    "sfw_cycle_kernelIdLb0ELb1E": (132, 136, 3),
    "sfw_cycle_kernelIdLb1ELb1E": (124, 136, 4),
    "sfw_batch_cycle_kernelIdLb0ELb0E": (85, 136, 5),
    "sfw_batch_cycle_kernelIdLb0ELb1E": (132, 136, 3),
    "sfw_batch_cycle_kernelIdLb1ELb1E": (124, 136, 4),
}
PARENT_FIGURES_F32 = {  # (the strict unit is f64 only)
    "sfw_social_kernelIfLi1ELb0E": (63, 0, 7),
    "sfw_social_kernel_flatIfLb0ELi64ELb0E": (66, 0, 7),
    "sfw_social_kernel_mixedIf": (67, 0, 7),
    "sfw_cycle_kernelIfLb0ELb0E": (83, 136, 5),
    "sfw_batch_cycle_kernelIfLb0ELb0E": (83, 136, 5),
}


@pytest.mark.parametrize("tu", TUS)
def test_resource_figures_equal_the_parents(tu):
    res = listing(tu).resources
    want = dict(PARENT_FIGURES, **(PARENT_FIGURES_F32 if tu == TUS[0] else {}))
    got = {}
    for name in want:
        k = one(res, name)
        got[name] = (k["vgpr"], k["scratch"], k["occupancy"])
    assert got == want
