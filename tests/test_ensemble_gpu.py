"""sfw_ensemble_* (one grid under several crowd hypotheses).

Every case runs on the reference's 5 x 9 grid (the members take the one-launch cycle, batched) and on a 48 x 48 cfg2-style
grid (too many samples for it: the members' usual kernels).  The ensemble must equal what its definition computes from the
members' own captured terms (include/sfw_hip.h), bit for bit, and what the CPU oracle computes, within the parity tolerance."""
import ctypes as C
import dataclasses
import math
from fractions import Fraction

import numpy as np
import pytest

from social_force_window_planner_amd import synthetic as syn
from social_force_window_planner_amd._abi import (SFW_COST_INVALID, SFW_COST_SKIPPED, SFW_ERR_INVALID_ARG, SFW_ERR_STATE,
                                                   SFW_PRECISION_F32, SFW_PRECISION_F64, SFW_PRECISION_F64_STRICT, SfwAgent,
                                                   SfwBest)
from social_force_window_planner_amd.hypotheses import naive_goal_hypotheses
from sfw_test_util import _same, _scene_params as _params

pytestmark = pytest.mark.gpu

RTOL_F64 = 1e-9  # tests/test_parity_gpu.py
WEIGHT_FIELDS = ("vel_weight", "distance_weight", "angle_weight", "costmap_weight", "social_weight")
GRIDS = ("ref5x9", "cfg2_48")


def _scene(name):
    if name == "ref5x9":
        return syn.make_scene("ref5x9")
    return syn.make_scene(dataclasses.replace(syn.WORKLOADS["cfg2"], nv=48, nw=48, n_people=8))


def _grid_args(scene):
    return scene.robot_state, scene.linvels, scene.angvels, scene.goal_args


def _ensemble(hip_mod, scene, hypotheses, params=None):
    e = hip_mod.EnsembleScorer(params if params is not None else _params(scene), 0, len(hypotheses))
    e.load_scene(scene, hypotheses)
    return e


def _standalone(hip_mod, scene, agents, obstacles, params=None):
    g = hip_mod.HipScorer(params if params is not None else _params(scene))
    g.load_scene(scene)
    g.set_agents(agents, obstacles)
    return g


def _with_person(agents, x, y, vx, vy):
    out = (SfwAgent * (len(agents) + 1))()
    for i, a in enumerate(agents):
        C.memmove(C.byref(out[i]), C.byref(a), C.sizeof(SfwAgent))
    p = out[len(agents)]
    p.x, p.y, p.vx, p.vy = x, y, vx, vy
    p.goal_x, p.goal_y = x + 2.0 * vx, y + 2.0 * vy
    p.goal_radius = p.radius = 0.35
    p.desired_velocity, p.has_goal, p.id, p.group_id = 1.0, 1, 90, -1
    return out


def _laser(n):
    a = np.arange(n) * (2.0 * math.pi / n)
    return np.stack([2.5 * np.cos(a), 1.5 + 0.4 * np.sin(a)], axis=1)


def _mixed_hypotheses(scene):
    """4 naive-goal hypotheses, one with a person added, one with 60 laser points (M = 6)"""
    hyps = [(h, scene.obstacles) for h in naive_goal_hypotheses(scene.agents, (1.0, 3.0), (0.0, 0.5))]
    hyps.append((_with_person(scene.agents, 1.5, -0.6, -0.3, 0.6), scene.obstacles))
    hyps.append((naive_goal_hypotheses(scene.agents, (2.0,))[0], _laser(60)))
    return hyps


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _host_ensemble(terms, weights, mode, probs=None):
    """The definition (include/sfw_hip.h) from the members' captured terms: costs, rejected"""
    M, T = len(terms), terms[0].shape[0]
    D = np.stack([t[:, 1] for t in terms])
    W = np.stack([t[:, 4] for t in terms])
    rejected = (D == SFW_COST_INVALID).sum(axis=0).astype(np.int32)
    skipped = np.any(D == SFW_COST_SKIPPED, axis=0)
    rejected[skipped] = 0
    if mode == "mean":
        p = np.full(M, 1.0 / M) if probs is None else np.asarray(probs, dtype=np.float64)
        acc = np.zeros(T)
        for m in range(M):
            acc = acc + p[m] * W[m]  # (numpy: every product and sum rounded on its own)
    else:
        acc = W.max(axis=0)
    wv, wd, wa, wc, ws = weights
    t0 = terms[0]
    base = wv * t0[:, 0] + wd * t0[:, 1] + wa * t0[:, 2]
    base = base + wc * t0[:, 3]
    costs = np.array([_fma(ws, acc[t], base[t]) for t in range(T)])
    costs[rejected > 0] = SFW_COST_INVALID
    costs[skipped] = SFW_COST_SKIPPED
    return costs, rejected


def _weights(p):
    return tuple(getattr(p, f) for f in WEIGHT_FIELDS)


# ---- 1. M = 1, MEAN with p = {1}: the standalone handle's results ----------------------------------------------------------
def _check_single(hip_mod, scene, precision):
    p = _params(scene, precision)
    e = _ensemble(hip_mod, scene, [(scene.agents, scene.obstacles)], p)
    costs, rejected, best = e.score_grid(*_grid_args(scene), mode="mean", probs=[1.0])
    g = _standalone(hip_mod, scene, scene.agents, scene.obstacles, p)
    gc, gb = g.score_grid(*_grid_args(scene))
    assert _same(costs, gc), f"{int(np.sum(costs != gc))} costs differ"
    assert best == gb
    assert np.array_equal(rejected, (gc == SFW_COST_INVALID).astype(np.int32))
    assert _same(e.member(0).costs_view(), gc)
    e.close()
    g.close()
    return costs


@pytest.mark.parametrize("grid", GRIDS)
def test_single_member_is_the_standalone_handle(hip_mod, grid):
    costs = _check_single(hip_mod, _scene(grid), SFW_PRECISION_F64)
    assert np.any(costs >= 0)
    assert np.any(costs == SFW_COST_SKIPPED) == (grid == "ref5x9")  # (an even nw has no zero angular velocity)


# ---- 2. M copies under MAX ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_copies_under_max_are_the_standalone_handle(hip_mod, grid):
    scene = _scene(grid)
    M = 4
    e = _ensemble(hip_mod, scene, [(scene.agents, scene.obstacles)] * M)
    costs, rejected, best = e.score_grid(*_grid_args(scene), mode="max")
    g = _standalone(hip_mod, scene, scene.agents, scene.obstacles)
    gc, gb = g.score_grid(*_grid_args(scene))
    assert _same(costs, gc) and best == gb
    assert set(np.unique(rejected).tolist()) <= {0, M}
    assert np.array_equal(rejected == M, gc == SFW_COST_INVALID)
    for m in range(M):
        assert _same(e.member(m).costs_view(), gc)
    e.close()
    g.close()


# ---- 3. mixed hypotheses against the definition -------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("mode,probs", [("mean", None), ("mean", [0.5, 0.1, 0.1, 0.1, 0.15, 0.3]), ("max", None)])
def test_mixed_hypotheses_match_the_definition(hip_mod, oracle_mod, grid, mode, probs):
    scene = _scene(grid)
    hyps = _mixed_hypotheses(scene)
    M = len(hyps)
    p = _params(scene)
    e = _ensemble(hip_mod, scene, hyps, p)
    costs, rejected, best = e.score_grid(*_grid_args(scene), mode=mode, probs=probs)
    terms = [e.member(m).cost_terms() for m in range(M)]
    hc, hr = _host_ensemble(terms, _weights(p), mode, probs)
    assert np.array_equal(rejected, hr)
    assert _same(costs, hc), f"{int(np.sum(costs != hc))} costs differ"
    assert best == oracle_mod.select_best(scene.linvels, scene.angvels, hc)
    assert best["n_valid"] == int(np.sum(hc >= 0))
    # the pedestrian-free terms do not depend on the agents
    accepted = rejected == 0
    accepted &= costs != SFW_COST_SKIPPED
    assert accepted.any()
    for m in range(1, M):
        assert _same(terms[m][accepted, :4], terms[0][accepted, :4]), f"member {m}"
    assert len({e.member(m).plan_info()["one_launch"] for m in range(M)}) == 1
    assert e.member(0).plan_info()["one_launch"] == (grid == "ref5x9")
    e.close()


# ---- 4. against the CPU oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_against_the_oracle(hip_mod, oracle_mod, grid):
    scene = _scene(grid)
    hyps = _mixed_hypotheses(scene)
    hyps = hyps[:3] + hyps[4:5]  # (three naive-goal crowds and the one with a person added)
    M = len(hyps)
    p = _params(scene)
    e = _ensemble(hip_mod, scene, hyps, p)
    probs = [0.4, 0.3, 0.2, 0.1]
    results = {"mean": e.score_grid(*_grid_args(scene), mode="mean", probs=probs), "max": e.aggregate("max")}
    full, social = [], []
    for agents, obs in hyps:
        for dst, prm in ((full, p), (social, _params(scene, vel_weight=0.0, distance_weight=0.0, angle_weight=0.0, costmap_weight=0.0,
                                                    social_weight=1.0))):
            o = oracle_mod.OracleScorer(prm)
            o.load_scene(scene)
            o.set_agents(agents, obs)
            c, _ = o.score_grid(*_grid_args(scene), n_threads=8)
            dst.append(c)
            o.close()
    Cf, W = np.stack(full), np.stack(social)
    rej = (Cf == SFW_COST_INVALID).sum(axis=0)
    skipped = Cf[0] == SFW_COST_SKIPPED
    rej[skipped] = 0
    base = Cf[0] - p.social_weight * W[0]  # (a member that accepts: the pedestrian-free part of its cost)
    for mode, agg in (("mean", sum(probs[m] * W[m] for m in range(M))), ("max", W.max(axis=0))):
        oc = np.where(rej > 0, SFW_COST_INVALID, base + p.social_weight * agg)
        oc[skipped] = SFW_COST_SKIPPED
        gc, gr, gb = results[mode]
        assert np.array_equal(gr, rej)
        assert np.array_equal(gc < 0, oc < 0) and np.array_equal(gc[gc < 0], oc[oc < 0]), "sentinel sets differ"
        v = oc >= 0
        rel = np.abs(gc[v] - oc[v]) / np.abs(oc[v])
        assert rel.max() <= RTOL_F64, f"{mode}: max rel err {rel.max():.3e}"
        ob = oracle_mod.select_best(scene.linvels, scene.angvels, oc)
        assert (gb["index"], gb["vx"], gb["vtheta"], gb["n_valid"]) == (ob["index"], ob["vx"], ob["vtheta"], ob["n_valid"])
    e.close()


# ---- 5. a hypothesis that puts a person into the straight-ahead samples -------------------------------------------------
def _straight_ahead(scene):
    cols = np.abs(scene.angvels) == np.abs(scene.angvels).min()
    return np.flatnonzero(np.tile(cols, len(scene.linvels)))


@pytest.mark.parametrize("grid", GRIDS)
def test_crossing_hypothesis_changes_the_command(hip_mod, grid):
    # a person ahead of the robot walking away from it; the second hypothesis turns its heading round: head-on
    scene = _scene(grid)
    hyps = naive_goal_hypotheses(_with_person(scene.agents, 1.6, 0.1, 1.3, 0.0), (2.0,), (0.0, math.pi))
    M = len(hyps)
    e = _ensemble(hip_mod, scene, [(h, scene.obstacles) for h in hyps])
    g = _standalone(hip_mod, scene, hyps[0], scene.obstacles)
    _, nominal = g.score_grid(*_grid_args(scene))
    costs, rejected, best = e.score_grid(*_grid_args(scene), mode="mean")
    straight = _straight_ahead(scene)
    assert np.any((rejected[straight] > 0) & (rejected[straight] < M)), "no straight-ahead sample rejected by some crowds only"
    assert rejected[nominal["index"]] > 0 and costs[nominal["index"]] == SFW_COST_INVALID
    assert best["index"] >= 0 and best["index"] != nominal["index"]
    assert np.all(costs[rejected > 0] == SFW_COST_INVALID) and np.all(rejected[costs == SFW_COST_SKIPPED] == 0)
    e.close()
    g.close()


@pytest.mark.parametrize("grid", GRIDS)
def test_mean_and_max_pick_different_commands(hip_mod, grid):
    # the people's headings turned by +-0.8 rad: the average crowd and the worst crowd favour different commands
    scene = _scene(grid)
    hyps = naive_goal_hypotheses(scene.agents, (2.0,), (0.0, 0.8, -0.8))
    e = _ensemble(hip_mod, scene, [(h, scene.obstacles) for h in hyps])
    costs, rejected, mean_best = e.score_grid(*_grid_args(scene), mode="mean")
    mc, mr, max_best = e.aggregate("max")
    assert mean_best["index"] >= 0 and max_best["index"] >= 0
    assert max_best["index"] != mean_best["index"], "MEAN and MAX pick the same command"
    assert np.array_equal(mr, rejected) and np.array_equal(mc < 0, costs < 0)
    v = costs >= 0
    assert np.all(mc[v] >= costs[v]), "the worst case costs at least the mean"
    assert e.aggregate("mean")[2] == mean_best
    e.close()


# ---- 6. aggregate == score_grid, and the state rules ----------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_aggregate_equals_score_grid_and_state_rules(hip_mod, grid):
    scene = _scene(grid)
    hyps = [(h, scene.obstacles) for h in naive_goal_hypotheses(scene.agents, (1.0, 2.0, 3.0))]
    e = _ensemble(hip_mod, scene, hyps)
    probs = [0.2, 0.5, 0.3]
    with pytest.raises(hip_mod.SfwError) as ex:
        e.aggregate("mean")
    assert ex.value.status == SFW_ERR_STATE  # nothing scored
    ref = {mode: e.score_grid(*_grid_args(scene), mode=mode, probs=probs) for mode in ("max", "mean")}
    for mode in ("max", "mean"):
        c, r, b = e.aggregate(mode, probs)
        rc, rr, rb = ref[mode]
        assert _same(c, rc) and np.array_equal(r, rr) and b == rb
    # bad arguments: before any device call
    for mode, probs_bad in ((7, None), ("mean", [0.5, -0.1, 0.6]), ("mean", [0.5, float("nan"), 0.5]), ("max", [float("inf"), 0, 0])):
        with pytest.raises(hip_mod.SfwError) as ex:
            e.aggregate(mode, probs_bad)
        assert ex.value.status == SFW_ERR_INVALID_ARG
        with pytest.raises(hip_mod.SfwError) as ex:
            e.score_grid(*_grid_args(scene), mode=mode, probs=probs_bad)
        assert ex.value.status == SFW_ERR_INVALID_ARG
    assert e.aggregate("mean")[2] == e.score_grid(*_grid_args(scene))[2]
    # a member staged since the last score
    e.member(1).stage(*_grid_args(scene))
    with pytest.raises(hip_mod.SfwError) as ex:
        e.aggregate("mean")
    assert ex.value.status == SFW_ERR_STATE
    e.score_grid(*_grid_args(scene))
    e.aggregate("max")
    # ... staged and launched on its own
    m2 = e.member(2)
    m2.stage(*_grid_args(scene))
    m2.launch()
    m2.fetch()
    with pytest.raises(hip_mod.SfwError) as ex:
        e.aggregate("mean")
    assert ex.value.status == SFW_ERR_STATE
    e.score_grid(*_grid_args(scene))
    # ... used for sfw_score_one
    e.member(0).score_one(scene.robot_state, 0.3, 0.0, 0.1, scene.goal_args)
    with pytest.raises(hip_mod.SfwError) as ex:
        e.aggregate("mean")
    assert ex.value.status == SFW_ERR_STATE
    # parameters changed through a member handle
    e.member(1).set_params(_params(scene, social_weight=2.0))
    with pytest.raises(hip_mod.SfwError) as ex:
        e.score_grid(*_grid_args(scene))
    assert ex.value.status == SFW_ERR_STATE
    e.set_params(_params(scene))  # (replicated to every member again)
    e.score_grid(*_grid_args(scene))
    e.close()


def test_hypothesis_never_set(hip_mod):
    scene = _scene("ref5x9")
    e = hip_mod.EnsembleScorer(_params(scene), 0, 3)
    e.set_costmap(scene.cells, scene.origin_x, scene.origin_y, scene.resolution)
    e.set_footprint(scene.footprint)
    e.set_hypothesis(0, scene.agents)
    e.set_hypothesis(2, scene.agents)
    with pytest.raises(hip_mod.SfwError) as ex:
        e.score_grid(*_grid_args(scene))
    assert ex.value.status == SFW_ERR_STATE and "hypothesis 1" in str(ex.value)
    with pytest.raises(hip_mod.SfwError) as ex:
        e.set_hypothesis(3, scene.agents)
    assert ex.value.status == SFW_ERR_INVALID_ARG
    e.set_hypothesis(1, scene.agents)
    _, _, best = e.score_grid(*_grid_args(scene))
    assert best["index"] >= 0
    e.close()


# ---- 7. precisions ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("precision", [SFW_PRECISION_F32, SFW_PRECISION_F64_STRICT])
def test_single_member_in_other_precisions(hip_mod, grid, precision):
    _check_single(hip_mod, _scene(grid), precision)


# ---- 8. lifetime --------------------------------------------------------------------------------------------------------
def test_lifetime_and_member_destroy_refused(hip_mod):
    scene = _scene("ref5x9")
    hyps = naive_goal_hypotheses(scene.agents, (1.0, 2.0, 3.0, 4.0), (0.0, 0.3, -0.3, 0.6))
    assert len(hyps) == 16
    L = hip_mod.lib()
    for _ in range(20):
        e = _ensemble(hip_mod, scene, [(h, scene.obstacles) for h in hyps])
        _, _, best = e.score_grid(*_grid_args(scene), mode="max")
        assert best["n_valid"] > 0
        assert L.sfw_ensemble_size(e._e) == 16
        assert L.sfw_ensemble_member(e._e, 16) is None and L.sfw_ensemble_member(e._e, -1) is None
        assert L.sfw_destroy(L.sfw_ensemble_member(e._e, 3)) == SFW_ERR_STATE
        us = e.last_us()
        assert us["enqueue"] > 0 and us["wait_fetch"] > 0
        e.close()
    b = SfwBest()
    assert L.sfw_ensemble_aggregate(None, 0, None, None, None, C.byref(b)) == SFW_ERR_INVALID_ARG
