"""Sample lists (sfw_samples_stage / sfw_score_samples): one launch scores arbitrary (vx, vy, vtheta) commands.

The contract under test: costs[t] is bit for bit what the scalar call returns for sample t — hence bit for bit the grid's cost
wherever the list holds a grid product — and within RTOL_F64 of the CPU oracle; the list has no hidden product structure; the
selection is the reference's rule over the list; and everything that acts on a staged grid (plan_info, points, terms, re-score,
batches, the stage / launch state machine) acts on a staged list.  "Bitwise" compares the uint64 views of the cost vectors."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from social_force_window_planner_amd import synthetic as syn
from social_force_window_planner_amd._abi import (SFW_COST_INVALID, SFW_COST_SKIPPED, SFW_ERR_INVALID_ARG, SFW_ERR_STATE,
                                                   SFW_K2_AUTO, SFW_K2_FLAT, SFW_ORG_REGISTER_2, SFW_PRECISION_F32,
                                                   SFW_PRECISION_F64, SFW_PRECISION_F64_STRICT, default_params)
from sfw_test_util import _np_best, _same

pytestmark = pytest.mark.gpu

RTOL_F64 = 1e-9  # the project's parity tolerance (tests/test_parity_gpu.py)
HOLO_GA = (1.0, 0.7, 1.0, 2.0, 0.5)
S = 40  # every workload here: sim_time 1.0 at 0.025


def _scorer(hip_mod, scene, precision=SFW_PRECISION_F64, form=SFW_K2_AUTO):
    g = hip_mod.HipScorer(default_params(precision=precision))
    g.load_scene(scene)
    if form != SFW_K2_AUTO:
        g.set_k2_form(form)
    return g


def _products(scene):
    """all nv * nw products of a scene's axes, grid order"""
    vx = np.repeat(scene.linvels, len(scene.angvels))
    vth = np.tile(scene.angvels, len(scene.linvels))
    return vx, vth


def _grid_as_list_reference(hip_mod, scene, precision=SFW_PRECISION_F64):
    """the grid's costs with the skipped (0,0) sample replaced by the scalar call's cost for (0, 0, 0)"""
    g = _scorer(hip_mod, scene, precision)
    gc, _ = g.score_grid(scene.robot_state, scene.linvels, scene.angvels, scene.goal_args)
    skipped = np.flatnonzero(gc == SFW_COST_SKIPPED)
    assert skipped.size == 1
    ref = gc.copy()
    ref[skipped[0]], _ = g.score_one(scene.robot_state, 0.0, 0.0, 0.0, scene.goal_args)
    g.close()
    return ref


# ---- 1. the grid as a list, on the one-launch kernel (and on the fused K1 + K2 + K3 without it) -----------------------------------
@pytest.mark.parametrize("fused", [True, False])
def test_grid_as_list_ref5x9(hip_mod, monkeypatch, fused):
    monkeypatch.setenv("SFW_CYCLE_FUSED", "1" if fused else "0")
    scene = syn.make_scene("ref5x9")
    ref = _grid_as_list_reference(hip_mod, scene)
    vx, vth = _products(scene)
    g = _scorer(hip_mod, scene)
    g.stage_samples(scene.robot_state, vx, vth, scene.goal_args)
    plan = g.plan_info()
    assert plan["one_launch"] == (1 if fused else 0) and plan["levels"] == 0 and plan["samples"] == 45, plan
    assert plan["split_step"] == 0 and plan["classes"] == 0 and plan["class_steps"] == 0 and plan["chunks"] == 1, plan
    g.launch()
    costs, best, _ = g.fetch()
    assert _same(costs, ref), np.flatnonzero(costs != ref)
    assert not np.any(costs == SFW_COST_SKIPPED) and not np.any(np.isnan(costs))
    assert best == _np_best(costs, vx, None, vth)
    # vy given as zeros is the same list
    c0, b0 = g.score_samples(scene.robot_state, vx, vth, scene.goal_args, vy=np.zeros_like(vx))
    assert _same(c0, ref) and b0 == best
    g.close()


# ---- 2. no hidden product structure --------------------------------------------------------------------------------------
def _permuted(scene):
    vx, vth = _products(scene)
    rng = np.random.default_rng(5)
    perm = rng.permutation(vx.size)
    perm = np.concatenate([perm, perm[[3, 11, 17, 29, 40]]])  # five duplicates: N = 50
    return perm, vx[perm], vth[perm]


def test_permuted_list_with_duplicates(hip_mod):
    scene = syn.make_scene("ref5x9")
    ref = _grid_as_list_reference(hip_mod, scene)
    perm, vx, vth = _permuted(scene)
    assert vx.size == 50
    g = _scorer(hip_mod, scene)
    costs, best = g.score_samples(scene.robot_state, vx, vth, scene.goal_args)
    assert _same(costs, ref[perm]), np.flatnonzero(costs != ref[perm])
    assert best == _np_best(costs, vx, None, vth)
    g.close()


# ---- 7. precision modes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [SFW_PRECISION_F32, SFW_PRECISION_F64_STRICT])
def test_permuted_list_precision_modes(hip_mod, precision):
    scene = syn.make_scene("ref5x9")
    ref = _grid_as_list_reference(hip_mod, scene, precision)
    perm, vx, vth = _permuted(scene)
    g = _scorer(hip_mod, scene, precision)
    costs, best = g.score_samples(scene.robot_state, vx, vth, scene.goal_args)
    assert _same(costs, ref[perm]), np.flatnonzero(costs != ref[perm])
    assert best == _np_best(costs, vx, None, vth)
    g.close()


# ---- 3. holonomic, against the oracle -----------------------------------------------------------------------------------------
def _holo_scene(n_people=8):
    return syn.make_scene(dataclasses.replace(syn.WORKLOADS["cfg2"], n_people=n_people, seed=12))


def _holo_samples():
    rng = np.random.default_rng(123)
    vx = rng.uniform(0.0, 0.7, 64)
    vy = rng.uniform(-0.3, 0.3, 64)
    vth = rng.uniform(-0.5, 0.5, 64)
    return vx, vy, vth


@pytest.mark.parametrize("n_people,form,min_valid", [(8, SFW_K2_AUTO, 60), (70, SFW_K2_AUTO, 50), (8, SFW_K2_FLAT, 60)])
def test_holonomic_list_against_oracle_and_score_one(oracle_mod, hip_mod, n_people, form, min_valid):
    scene = _holo_scene(n_people)
    vx, vy, vth = _holo_samples()
    o = oracle_mod.OracleScorer(default_params())
    o.load_scene(scene)
    oc = np.array([o.score_one(scene.robot_state, vx[t], vy[t], vth[t], HOLO_GA)[0] for t in range(64)])
    g = _scorer(hip_mod, scene, form=form)
    costs, best = g.score_samples(scene.robot_state, vx, vth, HOLO_GA, vy=vy)
    assert not np.any(np.isnan(costs)) and not np.any(costs == SFW_COST_SKIPPED)
    assert np.array_equal(oc < 0, costs < 0) and np.array_equal(oc[oc < 0], costs[costs < 0]), "sentinel sets differ"
    v = oc >= 0
    assert int(v.sum()) >= min_valid
    rel = np.abs(costs[v] - oc[v]) / np.abs(oc[v])
    print(f"holonomic list, {n_people} people: {int(v.sum())} valid, max rel err {rel.max():.3e}")
    assert rel.max() <= RTOL_F64
    one = np.array([g.score_one(scene.robot_state, vx[t], vy[t], vth[t], HOLO_GA)[0] for t in range(64)])
    assert _same(costs, one), np.flatnonzero(costs != one)
    assert best == _np_best(costs, vx, vy, vth) and best["n_valid"] == int(v.sum())
    if n_people == 70:  # (the oracle rejects 6 of the 64 by pedestrian contact; 64 samples alone run the flat form: the
        # two-slot register form is forced in the test below)
        assert int((oc == SFW_COST_INVALID).sum()) == 6 and int(v.sum()) == 58
    else:
        assert int(v.sum()) == 64
    g.close()


def test_holonomic_list_register_form_two_slots(hip_mod):
    """64 < A <= 128 in the register form with two agent slots per lane (forced: 64 samples alone would run flat)."""
    from social_force_window_planner_amd._abi import SFW_K2_REGISTER
    scene = _holo_scene(70)
    vx, vy, vth = _holo_samples()
    g = _scorer(hip_mod, scene)
    auto, _ = g.score_samples(scene.robot_state, vx, vth, HOLO_GA, vy=vy)
    g.set_k2_form(SFW_K2_REGISTER)
    g.stage_samples(scene.robot_state, vx, vth, HOLO_GA, vy=vy)
    assert g.plan_info()["organisation"] == SFW_ORG_REGISTER_2
    g.launch()
    reg, _, _ = g.fetch()
    assert _same(auto, reg)
    g.close()


# ---- 4. costmap rejection and points ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capture", [True, False])
def test_costmap_rejection_and_points(hip_mod, capture):
    scene = _holo_scene(8)
    scene.cells[:, 110:114] = 254
    # (0.7, 0, 0) drives into the wall; the CPU oracle scores the other four >= 0 with all 40 poses legal
    vx = np.array([0.1, 0.7, 0.0, 0.05, 0.1])
    vy = np.array([-0.2, 0.0, 0.25, -0.3, 0.2])
    vth = np.array([-0.4, 0.0, 0.1, 0.3, -0.5])
    g = _scorer(hip_mod, scene)
    g.set_points_capture(capture)
    costs, best = g.score_samples(scene.robot_state, vx, vth, HOLO_GA, vy=vy)
    assert costs[1] == SFW_COST_INVALID and np.all(np.delete(costs, 1) >= 0), costs
    assert best == _np_best(costs, vx, vy, vth) and best["n_valid"] == 4
    pts, n = g.grid_points_batch(0, 5, S)
    h = _scorer(hip_mod, scene)
    for t in range(5):
        c1, p1 = h.score_one(scene.robot_state, vx[t], vy[t], vth[t], HOLO_GA)
        assert _same([c1], [costs[t]])
        assert n[t] == len(p1) and _same(pts[t, :n[t]], p1), t
    assert 0 < n[1] < S and np.all(np.delete(n, 1) == S)
    g.close()
    h.close()


# ---- 5. the three-kernel rollout ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cfg2_grid(hip_mod):
    scene = syn.make_scene("cfg2")
    g = _scorer(hip_mod, scene)
    gc, _ = g.score_grid(scene.robot_state, scene.linvels, scene.angvels, scene.goal_args)
    assert g.plan_info()["levels"] > 0  # (the grid itself shares a prefix)
    g.close()
    return scene, gc


def _random_pairs(scene, n, seed):
    rng = np.random.default_rng(seed)
    iv = rng.integers(0, len(scene.linvels), n)
    iw = rng.integers(0, len(scene.angvels), n)
    return iv, iw


@pytest.mark.parametrize("n", [2100, 4100])
def test_large_list_equals_grid(hip_mod, cfg2_grid, n):
    scene, gc = cfg2_grid
    iv, iw = _random_pairs(scene, n, 77)
    g = _scorer(hip_mod, scene)
    g.stage_samples(scene.robot_state, scene.linvels[iv], scene.angvels[iw], scene.goal_args)
    plan = g.plan_info()
    assert plan["samples"] == n and plan["levels"] == 0 and plan["one_launch"] == 0 and plan["chunks"] == 1, plan
    g.launch()
    costs, best, _ = g.fetch()
    want = gc[iv * len(scene.angvels) + iw]
    keep = want != SFW_COST_SKIPPED
    assert keep.sum() >= n - 8 and _same(costs[keep], want[keep]), np.flatnonzero(costs != want)
    assert not np.any(costs == SFW_COST_SKIPPED)
    assert best == _np_best(costs, scene.linvels[iv], None, scene.angvels[iw])
    g.close()


def test_large_list_chunked(hip_mod, cfg2_grid, monkeypatch):
    scene, gc = cfg2_grid
    iv, iw = _random_pairs(scene, 2100, 77)
    g1 = _scorer(hip_mod, scene)
    c1, b1 = g1.score_samples(scene.robot_state, scene.linvels[iv], scene.angvels[iw], scene.goal_args)
    monkeypatch.setenv("SFW_TABLE_BUDGET_MB", "1")  # 1 MiB -> chunk floor of 1024 samples < 2100
    g2 = _scorer(hip_mod, scene)
    g2.stage_samples(scene.robot_state, scene.linvels[iv], scene.angvels[iw], scene.goal_args)
    assert g2.plan_info()["chunks"] > 1
    g2.launch()
    c2, b2, _ = g2.fetch()
    assert _same(c1, c2) and b1 == b2
    g1.close()
    g2.close()


# ---- 6. laser points and groups ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [False, True])
def test_laser_points_and_groups(hip_mod, groups):
    scene = syn.make_scene(dataclasses.replace(syn.WORKLOADS["cfg2"], nv=12, nw=12, n_people=8, n_obstacles=8))
    if groups:
        for a in range(1, min(len(scene.agents) - 1, 7) + 1):
            scene.agents[a].group_id = 1 + (a % 2)
    g = _scorer(hip_mod, scene)
    gc, _ = g.score_grid(scene.robot_state, scene.linvels, scene.angvels, scene.goal_args)
    iv, iw = _random_pairs(scene, 40, 9)
    costs, best = g.score_samples(scene.robot_state, scene.linvels[iv], scene.angvels[iw], scene.goal_args)
    want = gc[iv * 12 + iw]
    keep = want != SFW_COST_SKIPPED
    assert keep.sum() >= 38 and _same(costs[keep], want[keep]), np.flatnonzero(costs != want)
    assert best == _np_best(costs, scene.linvels[iv], None, scene.angvels[iw])
    g.close()


# ---- 8. selection ------------------------------------------------------------------------------------------------------------
def test_duplicated_winner_and_index_base(hip_mod):
    scene = _holo_scene(8)
    vx, vy, vth = _holo_samples()
    g = _scorer(hip_mod, scene)
    costs, best = g.score_samples(scene.robot_state, vx, vth, HOLO_GA, vy=vy)
    w = best["index"]
    assert 0 <= w < 64
    # a copy of the winner with another vy and a cost that may differ takes no part: an EXACT copy appended wins by its index
    vx2, vy2, vth2 = np.append(vx, vx[w]), np.append(vy, vy[w]), np.append(vth, vth[w])
    c2, b2 = g.score_samples(scene.robot_state, vx2, vth2, HOLO_GA, vy=vy2)
    assert _same(c2[:64], costs) and _same([c2[64]], [costs[w]])
    assert b2["index"] == 64 and b2["cost"] == best["cost"] and b2["n_valid"] == best["n_valid"] + 1
    assert (b2["vx"], b2["vy"], b2["vtheta"]) == (vx[w], vy[w], vth[w])
    assert b2 == _np_best(c2, vx2, vy2, vth2)
    g.stage_samples(scene.robot_state, vx, vth, HOLO_GA, vy=vy, index_base=1000)
    g.launch()
    c3, b3, key = g.fetch()
    assert _same(c3, costs) and b3 == best
    assert key == (best["cost"], -vx[w], abs(vth[w]), float(-(1000 + w)))
    g.close()


# ---- 9. terms and re-score -------------------------------------------------------------------------------------------------
def test_terms_and_rescore(hip_mod):
    scene = _holo_scene(70)  # (six of the 64 samples end in a pedestrian contact: sentinels in the terms)
    vx, vy, vth = _holo_samples()
    g = _scorer(hip_mod, scene)
    g.set_terms_capture(True)
    costs, best = g.score_samples(scene.robot_state, vx, vth, HOLO_GA, vy=vy)
    terms = g.cost_terms()
    assert terms.shape == (64, 5)
    sentinel = costs < 0
    assert sentinel.any() and np.all(terms[sentinel] == costs[sentinel][:, None])
    assert np.all(terms[~sentinel, 1] >= 0)
    weights = [(1.0, 1.0, 0.7, 2.0, 1.2), (0.2, 3.0, 0.0, 0.5, 4.0), (2.0, 0.5, -0.3, 1.0, 0.1)]
    bests, rc = g.rescore(weights, want_costs=True)
    for k, wv in enumerate(weights):
        p = default_params()
        p.vel_weight, p.distance_weight, p.angle_weight, p.costmap_weight, p.social_weight = wv
        f = hip_mod.HipScorer(p)
        f.load_scene(scene)
        fc, fb = f.score_samples(scene.robot_state, vx, vth, HOLO_GA, vy=vy)
        assert _same(rc[k], fc), (k, np.flatnonzero(rc[k] != fc))
        assert bests[k] == fb, (k, bests[k], fb)
        f.close()
    assert _same(rc[0], costs) and bests[0] == best
    g.close()


# ---- 10. state machine -------------------------------------------------------------------------------------------------------
def test_refused_stage_keeps_the_list(hip_mod):
    scene = _holo_scene(8)
    vx, vy, vth = _holo_samples()
    g = _scorer(hip_mod, scene)
    costs, best = g.score_samples(scene.robot_state, vx, vth, HOLO_GA, vy=vy)
    g.stage_samples(scene.robot_state, vx, vth, HOLO_GA, vy=vy)
    with pytest.raises(hip_mod.SfwError) as e:
        g.stage_samples(scene.robot_state, [], [], HOLO_GA)  # n = 0
    assert e.value.status == SFW_ERR_INVALID_ARG
    bad = vth.copy()
    bad[7] = np.nan
    with pytest.raises(hip_mod.SfwError) as e:
        g.stage_samples(scene.robot_state, vx, bad, HOLO_GA, vy=vy)
    assert e.value.status == SFW_ERR_INVALID_ARG
    bad_vy = vy.copy()
    bad_vy[0] = np.inf
    with pytest.raises(hip_mod.SfwError) as e:
        g.stage_samples(scene.robot_state, vx, vth, HOLO_GA, vy=bad_vy)
    assert e.value.status == SFW_ERR_INVALID_ARG
    L = hip_mod.lib()
    rs, ga = hip_mod.SfwRobotState(*scene.robot_state), hip_mod.SfwGoalArgs(*HOLO_GA)
    assert L.sfw_samples_stage(g._h, C.byref(rs), None, None, vth.ctypes.data, 64, C.byref(ga), 0) == SFW_ERR_INVALID_ARG
    assert L.sfw_samples_stage(g._h, C.byref(rs), vx.ctypes.data, None, vth.ctypes.data, 64, None, 0) == SFW_ERR_INVALID_ARG
    g._grid = (64, 1)
    g.launch()  # the first list is still staged
    c2, b2, _ = g.fetch()
    assert _same(c2, costs) and b2 == best
    g.close()


def test_list_and_grid_replace_each_other(hip_mod):
    scene = syn.make_scene("ref5x9")
    perm, vx, vth = _permuted(scene)
    g = _scorer(hip_mod, scene)
    gc, gb = g.score_grid(scene.robot_state, scene.linvels, scene.angvels, scene.goal_args)
    lc, lb = g.score_samples(scene.robot_state, vx, vth, scene.goal_args)
    g.stage_samples(scene.robot_state, vx, vth, scene.goal_args)
    g.stage(scene.robot_state, scene.linvels, scene.angvels, scene.goal_args)
    assert g.plan_info()["samples"] == 45
    g.launch()
    c, b, _ = g.fetch()
    assert _same(c, gc) and b == gb
    g.stage(scene.robot_state, scene.linvels, scene.angvels, scene.goal_args)
    g.stage_samples(scene.robot_state, vx, vth, scene.goal_args)
    assert g.plan_info()["samples"] == 50
    g.launch()
    c, b, _ = g.fetch()
    assert _same(c, lc) and b == lb
    # the scalar call consumes a staged list
    g.stage_samples(scene.robot_state, vx, vth, scene.goal_args)
    g.score_one(scene.robot_state, 0.3, 0.0, 0.1, scene.goal_args)
    with pytest.raises(hip_mod.SfwError) as e:
        g.launch()
    assert e.value.status == SFW_ERR_STATE
    g.close()


def test_no_costmap_is_a_state_error(hip_mod):
    g = hip_mod.HipScorer(default_params())
    with pytest.raises(hip_mod.SfwError) as e:
        g.stage_samples((0, 0, 0, 0, 0, 0), [0.1], [0.0], HOLO_GA)
    assert e.value.status == SFW_ERR_STATE
    g.close()


# ---- 11. batch -----------------------------------------------------------------------------------------------------------------
def test_batch_with_list_members(hip_mod):
    scene = syn.make_scene("ref5x9")
    perm, vx, vth = _permuted(scene)
    hvx, hvy, hvth = _holo_samples()
    rs, ga = scene.robot_state, scene.goal_args
    alone = _scorer(hip_mod, scene)
    want = [alone.score_samples(rs, vx, vth, ga), alone.score_grid(rs, scene.linvels, scene.angvels, ga),
            alone.score_samples(rs, hvx[:20], hvth[:20], HOLO_GA, vy=hvy[:20])]
    alone.close()
    bs = hip_mod.BatchScorer(default_params(), B=3)
    for i in range(3):
        bs.member(i).load_scene(scene)
    bs.member(0).stage_samples(rs, vx, vth, ga)
    bs.stage(1, rs, scene.linvels, scene.angvels, ga)
    bs.member(2).stage_samples(rs, hvx[:20], hvth[:20], HOLO_GA, vy=hvy[:20])
    bs.launch()
    bests = bs.fetch()
    for i in range(3):
        costs = bs.member(i).costs_view().copy()
        assert _same(costs, want[i][0]), (i, np.flatnonzero(costs != want[i][0]))
        assert bests[i] == want[i][1], (i, bests[i], want[i][1])
    d = bs.describe()
    assert d["members"] == 3 and d["one_launch_members"] + d["own_path_members"] == 3
    assert d["one_launch_members"] == 1 and d["own_path_members"] == 2, d  # the lists take their own (one-kernel) path
    bs.close()
