"""Per-term costs and re-scoring (sfw_set_terms_capture, sfw_grid_terms, sfw_grid_rescore).

A sample's cost is the weighted sum of five terms (reference src/sfw_planner.cpp:643-667).  With capture on, every launch
keeps the unweighted terms; term k must then be bit for bit the cost vector of a fresh launch under the unit weight vector
e_k (with the kernels' rounding, 0 * x + y and 1 * x + 0 are exact), a re-score under any weight vector bit for bit the
costs and field for field the selection of a fresh launch under those weights, and capturing must change nothing else."""
import dataclasses

import numpy as np
import pytest

from social_force_window_planner_amd import synthetic as syn
from social_force_window_planner_amd._abi import (SFW_COST_SKIPPED, SFW_ERR_INVALID_ARG, SFW_ERR_STATE, SFW_K2_AUTO,
                                                   SFW_K2_FLAT, SFW_K2_REGISTER, SFW_PRECISION_F32, SFW_PRECISION_F64,
                                                   SFW_PRECISION_F64_STRICT, SfwAgent, default_params)
from sfw_test_util import _same

pytestmark = pytest.mark.gpu

WEIGHT_FIELDS = ("vel_weight", "distance_weight", "angle_weight", "costmap_weight", "social_weight")


def _params(w, precision=SFW_PRECISION_F64, weights=None):
    p = default_params(sim_time=w.sim_time, sim_granularity=w.sim_granularity, precision=precision)
    if weights is not None:
        for f, v in zip(WEIGHT_FIELDS, weights):
            setattr(p, f, float(v))
    return p


def _weights_of(p):
    return [getattr(p, f) for f in WEIGHT_FIELDS]


def _workload(name, **kw):
    return dataclasses.replace(syn.WORKLOADS[name], **kw) if kw else syn.WORKLOADS[name]


def _scorer(hip_mod, scene, params, agents=None, form=SFW_K2_AUTO, capture=True):
    g = hip_mod.HipScorer(params)
    g.load_scene(scene)
    if agents is not None:
        g.set_agents(agents, None)
    if form != SFW_K2_AUTO:
        g.set_k2_form(form)
    g.set_terms_capture(capture)
    return g


def _score(g, scene):
    return g.score_grid(scene.robot_state, scene.linvels, scene.angvels, scene.goal_args)


def _with_groups(scene, n=7):
    for a in range(1, min(len(scene.agents) - 1, n) + 1):
        scene.agents[a].group_id = 1 + (a % 2)
    return scene


def _robot_alone(scene):
    return (SfwAgent * 1)(scene.agents[0])


def _check_terms_exact(hip_mod, scene, precision=SFW_PRECISION_F64, agents=None, form=SFW_K2_AUTO):
    """term k of a capturing launch == the costs of a fresh launch under e_k, bit for bit; returns the terms"""
    w = scene.workload
    g = _scorer(hip_mod, scene, _params(w, precision), agents, form)
    costs, best = _score(g, scene)
    terms = g.cost_terms()
    assert terms.shape == (costs.size, 5)
    sentinel = costs < 0
    assert np.all(terms[sentinel] == costs[sentinel][:, None]), "a sentinel sample must hold its sentinel in all five terms"
    for k in range(5):
        e = [0.0] * 5
        e[k] = 1.0
        g.set_params(_params(w, precision, e))
        ck, _ = _score(g, scene)
        assert _same(terms[:, k], ck), f"term {k} differs from the e_{k} launch ({int(np.sum(terms[:, k] != ck))} samples)"
    if agents is not None and len(agents) <= 1:  # (no laser points either: set_agents(agents, None))
        assert np.all(terms[~sentinel, 4] == 0.0)
    g.close()
    return costs, terms


def _cfg2(n_obs=0, nv=128, nw=128, **kw):
    return syn.make_scene(_workload("cfg2", n_obstacles=n_obs, nv=nv, nw=nw, **kw))


# ---- 1. terms are exact, at every write site ----------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
def test_terms_exact_ref5x9_cycle(hip_mod, monkeypatch, fused):
    monkeypatch.setenv("SFW_CYCLE_FUSED", "1" if fused else "0")
    scene = syn.make_scene("ref5x9")
    costs, terms = _check_terms_exact(hip_mod, scene)
    assert np.any(costs == SFW_COST_SKIPPED) and np.all(terms[costs == SFW_COST_SKIPPED] == SFW_COST_SKIPPED)
    _check_terms_exact(hip_mod, _with_groups(syn.make_scene("ref5x9")))
    _check_terms_exact(hip_mod, scene, agents=_robot_alone(scene))
    _check_terms_exact(hip_mod, scene, agents=(SfwAgent * 0)())


@pytest.mark.parametrize("n_obs", [0, 64, 240])
def test_terms_exact_cfg2_laser_points(hip_mod, n_obs):
    _check_terms_exact(hip_mod, _cfg2(n_obs))


@pytest.mark.parametrize("form", [SFW_K2_AUTO, SFW_K2_REGISTER, SFW_K2_FLAT])
def test_terms_exact_k2_forms(hip_mod, form):
    _check_terms_exact(hip_mod, _cfg2(0, nv=48, nw=48), form=form)


def test_terms_exact_groups_and_no_agents(hip_mod):
    _check_terms_exact(hip_mod, _with_groups(_cfg2(16, nv=40, nw=40)))
    scene = _cfg2(0, nv=40, nw=40)
    _check_terms_exact(hip_mod, scene, agents=(SfwAgent * 0)())
    _check_terms_exact(hip_mod, scene, agents=_robot_alone(scene))


@pytest.mark.parametrize("prefix", ["0", None])
def test_terms_exact_shared_prefix_on_off(hip_mod, monkeypatch, prefix):
    if prefix is None:
        monkeypatch.delenv("SFW_PREFIX", raising=False)
    else:
        monkeypatch.setenv("SFW_PREFIX", prefix)
    _check_terms_exact(hip_mod, _cfg2(0, nv=96, nw=96))


def test_terms_exact_chunked(hip_mod, monkeypatch):
    monkeypatch.setenv("SFW_TABLE_BUDGET_MB", "1")  # chunks of 1024 samples
    scene = _cfg2(16, nv=64, nw=48)
    g = hip_mod.HipScorer(_params(scene.workload))
    g.load_scene(scene)
    _score(g, scene)
    assert g.plan_info()["chunks"] > 1
    g.close()
    _check_terms_exact(hip_mod, scene)


@pytest.mark.parametrize("precision", [SFW_PRECISION_F64, SFW_PRECISION_F64_STRICT, SFW_PRECISION_F32])
def test_terms_exact_precisions(hip_mod, precision):
    _check_terms_exact(hip_mod, _cfg2(16, nv=48, nw=48), precision=precision)
    _check_terms_exact(hip_mod, syn.make_scene("ref5x9"), precision=precision)


# ---- 2. terms against the CPU oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene_fn", [lambda: syn.make_scene("ref5x9"), lambda: _with_groups(_cfg2(64, nv=16, nw=16))],
                         ids=["ref5x9", "cfg2_o64_groups_16x16"])
def test_terms_match_oracle(hip_mod, oracle_mod, scene_fn):
    scene = scene_fn()
    w = scene.workload
    g = _scorer(hip_mod, scene, _params(w))
    costs, _ = _score(g, scene)
    terms = g.cost_terms()
    g.close()
    o = oracle_mod.OracleScorer(_params(w))
    o.load_scene(scene)
    oc, _ = o.score_grid(scene.robot_state, scene.linvels, scene.angvels, scene.goal_args, n_threads=8)
    for k in range(5):
        e = [0.0] * 5
        e[k] = 1.0
        o.set_params(_params(w, weights=e))
        ok, _ = o.score_grid(scene.robot_state, scene.linvels, scene.angvels, scene.goal_args, n_threads=8)
        gk = terms[:, k]
        assert np.array_equal(ok < 0, gk < 0) and np.all(ok[ok < 0] == gk[gk < 0]), f"term {k}: sentinels differ"
        v = ok >= 0
        # the parity tests' 1e-9, relative to the term or to the sample's whole cost (a term far below the cost it is part of)
        scale = np.maximum(np.abs(ok[v]), np.abs(oc[v]))
        err = np.abs(gk[v] - ok[v])
        assert np.all(err <= 1e-9 * scale), f"term {k}: max err / scale {np.max(err / np.maximum(scale, 1e-300)):.3e}"


# ---- 3. re-score == fresh score -----------------------------------------------------------------------------------------
def _weight_set(terms, costs, rng, n_random=6):
    W = [list(rng.uniform(0.0, 3.0, 5)) for _ in range(n_random)]
    W.append([0.0] * 5)                       # everything ties: the tie-breaks decide
    W.append([1.0, -0.5, 0.7, 2.0, -1.2])    # negative weights: some valid samples become unselectable
    W.append([-1.0, -1.0, -1.0, -1.0, -1.0])
    W.append([1.0, 1e12, 0.7, 2.0, 1.2])     # distance_weight huge
    v = costs >= 0
    dist = terms[v, 1]
    if dist.size and dist.min() > 0:          # a cost exactly at 10000.0 as the minimum (distance term only): the == 10000 rule
        x = float(dist.min())
        wd = 10000.0 / x
        for _ in range(64):
            if np.float64(wd) * np.float64(x) == 10000.0:
                W.append([0.0, wd, 0.0, 0.0, 0.0])
                break
            wd = np.nextafter(wd, np.inf if np.float64(wd) * np.float64(x) < 10000.0 else -np.inf)
    return np.array(W, dtype=np.float64)


def _fresh(hip_mod, scene, params, W, stage_base=None):
    g = hip_mod.HipScorer(params)
    g.load_scene(scene)
    out = []
    for wk in W:
        g.set_params(_params(scene.workload, params.precision, wk))
        if stage_base is None:
            out.append(_score(g, scene))
        else:
            g.stage(scene.robot_state, scene.linvels, scene.angvels, scene.goal_args, index_base=stage_base)
            g.launch()
            c, b, _ = g.fetch()
            out.append((c, b))
    g.close()
    return out


@pytest.mark.parametrize("name", ["ref5x9", "cfg2_o64", "target"])
def test_rescore_equals_fresh_score(hip_mod, name):
    scene = syn.make_scene(name)
    p = _params(scene.workload)
    g = _scorer(hip_mod, scene, p)
    costs, best = _score(g, scene)
    terms = g.cost_terms()
    W = _weight_set(terms, costs, np.random.default_rng(11))
    if name == "ref5x9":
        assert any(w[1] > 1e3 and w[0] == 0.0 for w in W), "no 10000.0 vector built"
    bests, rc = g.rescore(W, want_costs=True)
    assert rc.shape == (len(W), costs.size)
    b1, none = g.rescore([_weights_of(p)])
    assert none is None and b1[0] == best
    assert _same(g.rescore([_weights_of(p)], want_costs=True)[1][0], costs)
    g.close()
    for k, (fc, fb) in enumerate(_fresh(hip_mod, scene, p, W)):
        assert _same(rc[k], fc), f"weights {W[k]}: costs differ at {int(np.sum(rc[k] != fc))} samples"
        assert bests[k] == fb, f"weights {W[k]}: {bests[k]} != {fb}"
    if name == "ref5x9":
        assert bests[-1]["cost"] == 10000.0 or bests[-1]["index"] == -1  # the == 10000 rule decided


def test_rescore_index_base_through_stage(hip_mod):
    scene = _cfg2(0, nv=24, nw=20)
    p = _params(scene.workload)
    g = _scorer(hip_mod, scene, p)
    g.stage(scene.robot_state, scene.linvels, scene.angvels, scene.goal_args, index_base=1000)
    g.launch()
    costs, best, _ = g.fetch()
    W = _weight_set(g.cost_terms(), costs, np.random.default_rng(5), n_random=3)
    bests, rc = g.rescore(W, want_costs=True)
    g.close()
    for k, (fc, fb) in enumerate(_fresh(hip_mod, scene, p, W, stage_base=1000)):
        assert _same(rc[k], fc) and bests[k] == fb


def test_rescore_many_weight_vectors(hip_mod):
    """K beyond one weight tile and up to SFW_RESCORE_MAX_K: every k as the same vector re-scored alone"""
    scene = _cfg2(0, nv=32, nw=32)
    g = _scorer(hip_mod, scene, _params(scene.workload))
    _score(g, scene)
    W = np.random.default_rng(3).uniform(-0.5, 3.0, (1024, 5))
    bests, rc = g.rescore(W, want_costs=True)
    for k in (0, 7, 8, 500, 1023):
        b, c = g.rescore(W[k:k + 1], want_costs=True)
        assert b[0] == bests[k] and _same(c[0], rc[k])
    g.close()


# ---- 4. capture is transparent ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ref5x9", "cfg2_o64"])
def test_capture_is_transparent(hip_mod, name):
    scene = syn.make_scene(name)
    p = _params(scene.workload)
    S = scene.workload.n_steps
    out = []
    for capture in (False, True):
        g = _scorer(hip_mod, scene, p, capture=capture)
        g.set_points_capture(True)
        costs, best = _score(g, scene)
        n = min(costs.size, 64)
        pts, npts = g.grid_points_batch(0, n, S)
        out.append((costs, best, pts, npts))
        if capture:  # a re-score leaves the launch's vector, selection and points as they were
            view0 = g.costs_view().copy()
            g.rescore(np.random.default_rng(1).uniform(0, 2, (20, 5)), want_costs=True)
            assert _same(g.costs_view(), view0) and _same(view0, costs)
            c2, b2, _ = g.fetch()
            assert _same(c2, costs) and b2 == best
            pts2, npts2 = g.grid_points_batch(0, n, S)
            assert _same(pts2, pts) and np.array_equal(npts2, npts)
        g.close()
    (c0, b0, p0, n0), (c1, b1, p1, n1) = out
    assert _same(c0, c1) and b0 == b1 and _same(p0, p1) and np.array_equal(n0, n1)


# ---- 5. state errors ----------------------------------------------------------------------------------------------------
def _status(fn):
    from social_force_window_planner_amd.planner import SfwError

    with pytest.raises(SfwError) as ei:
        fn()
    return ei.value.status


def test_state_errors_and_toggling(hip_mod):
    scene = syn.make_scene("ref5x9")
    sc2 = _cfg2(0, nv=12, nw=12)
    p = _params(scene.workload)
    g = _scorer(hip_mod, scene, p, capture=False)
    W = [[1, 1, 1, 1, 1]]
    _score(g, scene)
    assert _status(lambda: g.rescore(W)) == SFW_ERR_STATE
    assert _status(lambda: g.cost_terms()) == SFW_ERR_STATE
    g.set_terms_capture(True)
    _score(g, scene)
    g.rescore(W)
    assert _status(lambda: g.rescore([[np.nan, 1, 1, 1, 1]])) == SFW_ERR_INVALID_ARG
    assert _status(lambda: g.rescore(np.ones((1025, 5)))) == SFW_ERR_INVALID_ARG
    g.stage(scene.robot_state, scene.linvels, scene.angvels, scene.goal_args)
    assert _status(lambda: g.rescore(W)) == SFW_ERR_STATE
    g.launch()
    g.fetch()
    g.rescore(W)
    g.score_one(scene.robot_state, 0.2, 0.0, 0.1, scene.goal_args)
    assert _status(lambda: g.rescore(W)) == SFW_ERR_STATE
    assert _status(lambda: g.cost_terms()) == SFW_ERR_STATE
    # on, off, on across launches of different grids: never the terms of an earlier launch
    _score(g, sc2)
    g.set_terms_capture(False)
    _score(g, scene)
    assert _status(lambda: g.rescore(W)) == SFW_ERR_STATE
    g.set_terms_capture(True)
    _score(g, sc2)
    t_on = g.cost_terms()
    ref = _scorer(hip_mod, scene, p)  # (the same world and parameters as g: sc2's grid only)
    _score(ref, sc2)
    assert _same(t_on, ref.cost_terms())
    ref.close()
    # capture turned on between a stage and its launch
    g.set_terms_capture(False)
    g.stage(scene.robot_state, scene.linvels, scene.angvels, scene.goal_args)
    g.set_terms_capture(True)
    g.launch()
    g.fetch()
    ref = _scorer(hip_mod, scene, p)
    _score(ref, scene)
    assert _same(g.cost_terms(), ref.cost_terms())
    ref.close()
    g.close()


def test_capture_turned_on_between_stage_and_launch_large_grid(hip_mod):
    """a GPU-filling single-chunk grid whose pose rollout the stage enqueued before capture was on"""
    scene = _cfg2(0, nv=64, nw=64)
    p = _params(scene.workload)
    g = _scorer(hip_mod, scene, p, capture=False)
    g.stage(scene.robot_state, scene.linvels, scene.angvels, scene.goal_args)
    g.set_terms_capture(True)
    g.launch()
    g.fetch()
    ref = _scorer(hip_mod, scene, p)
    _score(ref, scene)
    assert _same(g.cost_terms(), ref.cost_terms())
    ref.close()
    g.close()


# ---- 6. batch -----------------------------------------------------------------------------------------------------------
# the mixed fleet of tests/test_batch_gpu.py: (people, laser points, nv, nw, steps, groups)
MIX = [(5, 0, 5, 9, 40, False), (0, 16, 3, 7, 6, False), (20, 60, 5, 9, 40, True), (1, 0, 32, 32, 6, False),
       (50, 240, 5, 9, 1, False), (62, 0, 3, 7, 40, False), (8, 16, 5, 9, 6, True)]


@dataclasses.dataclass
class Member:
    scene: object
    params: object
    robot_state: tuple
    goal_args: tuple


def _member(i, people, obs, nv, nw, steps, groups):
    gran = 0.025 if steps >= 40 else 0.25 if steps <= 6 else 0.05
    w = dataclasses.replace(syn.WORKLOADS["ref5x9"], n_people=people, n_obstacles=obs, sim_time=steps * gran,
                            sim_granularity=gran, seed=100 + 7 * i)
    if (nv, nw) != (5, 9):
        w = dataclasses.replace(w, nv=nv, nw=nw, sampler="generalised")
    scene = syn.make_scene(w)
    if groups:
        _with_groups(scene, min(people, 7))
    x, y, th, vx, vy, vth = scene.robot_state
    rs = (x + 0.01 * i, y - 0.005 * i, th + 0.02 * i, vx * (1.0 - 0.03 * (i % 5)), vy, vth + 0.01 * (i % 3))
    acc_x, acc_y, acc_th, wpx, wpy = scene.goal_args
    ga = (acc_x, acc_y, acc_th, wpx + 0.1 * (i % 4), wpy - 0.05 * (i % 3))
    return Member(scene, _params(w), rs, ga)


def test_batch_members_capture(hip_mod):
    members = [_member(i, *MIX[i]) for i in range(len(MIX))]
    bs = hip_mod.BatchScorer(members[0].params, B=len(members))
    for i, m in enumerate(members):
        h = bs.member(i)
        h.set_params(m.params)
        h.load_scene(m.scene)
        h.set_terms_capture(i % 2 == 0)
        bs.stage(i, m.robot_state, m.scene.linvels, m.scene.angvels, m.goal_args)
    bs.launch()
    bests = bs.fetch()
    for i, m in enumerate(members):
        g = hip_mod.HipScorer(m.params)
        g.load_scene(m.scene)
        g.set_terms_capture(True)
        costs, best = g.score_grid(m.robot_state, m.scene.linvels, m.scene.angvels, m.goal_args)
        h = bs.member(i)
        assert _same(h.costs_view(), costs) and bests[i] == best, f"member {i}"
        if i % 2 == 0:
            assert _same(h.cost_terms(), g.cost_terms()), f"member {i}: terms differ from its standalone launch"
            W = [[0.3, 1.0, 2.0, 0.5, 1.7], _weights_of(m.params)]
            assert h.rescore(W)[0] == g.rescore(W)[0]
        else:
            assert _status(lambda: h.cost_terms()) == SFW_ERR_STATE
        g.close()
    assert bs.describe()["one_launch_members"] > 0
    bs.close()


# ---- 7. lifetime --------------------------------------------------------------------------------------------------------
def test_create_capture_rescore_destroy_does_not_leak(hip_mod):
    import torch

    scene = _cfg2(16, nv=64, nw=64)
    p = _params(scene.workload)

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info(0)[0]

    def lap():
        g = _scorer(hip_mod, scene, p)
        _score(g, scene)
        g.rescore(np.ones((64, 5)), want_costs=True)
        g.cost_terms(0, 100)
        g.set_terms_capture(False)
        g.set_terms_capture(True)
        _score(g, scene)
        g.close()

    lap()
    f0 = free()
    for _ in range(6):
        lap()
    assert f0 - free() <= 4 << 20, f"device memory fell by {(f0 - free()) >> 20} MiB over six laps"
