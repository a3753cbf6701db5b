"""The predicted crowd behind a score (sfw_score_one_crowd / sfw_grid_crowd).

What is held to what:
  1. bitwise identities (uint64 views) with sfw_score_one / sfw_grid_points and between the two crowd calls, in all three
     precision modes;
  2. the work entries add up to the sample's social-work term (relative 2 A S 2^-53: every addend is non-negative, so any
     summation order is within (A S - 1) roundings of the exact sum);
  3. the captured state IS the reference's state: the CPU oracle continued from a captured row reproduces the rest of the
     social work (1e-9 relative, the project's parity tolerance);
  4. every work entry against the oracle's pair force evaluated on the captured rows;
  5. the rows are consistent with lightsfm's integrator (speed clamp, Euler step, goal pop);
  6. early ends (pedestrian contact, illegal footprint), steps_cap, argument and state checks.
Every scene is one wave of S = 32 steps with dt = 2^-5 exactly."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from social_force_window_planner_amd import synthetic as syn
from social_force_window_planner_amd._abi import (SFW_COST_SKIPPED, SFW_ERR_INVALID_ARG, SFW_ERR_STATE, SFW_PRECISION_F32,
                                                   SFW_PRECISION_F64, SFW_PRECISION_F64_STRICT, SfwAgent)
from sfw_test_util import _group_scene as _scene, _new_velocity, _params, _same, _scorer, _workload

pytestmark = pytest.mark.gpu

RTOL_F64 = 1e-9         # the project's parity tolerance (tests/test_parity_gpu.py)
RTOL_NORTH_STAR = 1e-4  # ... and its tolerance for SFW_PRECISION_F32
GRAN = 0.03125
S = 32
DT = 2.0 ** -5
PRECISIONS = [SFW_PRECISION_F64, SFW_PRECISION_F64_STRICT, SFW_PRECISION_F32]
F64_MODES = [SFW_PRECISION_F64, SFW_PRECISION_F64_STRICT]
# (people, seed, laser points): one person; the crowd sizes where the score path runs the register form and the flat form;
# 64 and more agents, where it is not the one-launch kernel; "group": 8 people, five of them in two groups
SCENE_KEYS = [(1, 11, 0), (5, 12, 0), (20, 13, 0), (20, 14, 16), (22, 17, 0), (40, 15, 0), (69, 16, 0), "group"]
PLAIN_KEYS = [k for k in SCENE_KEYS if k != "group" and k[2] == 0]  # no laser points, no groups
SAMPLES = [(0.5, 0.2), (0.1, -0.4), (0.7, 0.0)]
SOCIAL_ONLY = dict(vel_weight=0.0, distance_weight=0.0, angle_weight=0.0, costmap_weight=0.0, social_weight=1.0)
HOLO_GA = (1.0, 0.7, 1.0, 2.0, 0.5)


def _oracle(oracle_mod, scene, agents=None, sim_time=1.0, **kw):
    o = oracle_mod.OracleScorer(_params(sim_time=sim_time, **kw))
    o.set_costmap(scene.cells, scene.origin_x, scene.origin_y, scene.resolution)
    o.set_footprint(scene.footprint)
    o.set_agents(scene.agents if agents is None else agents, scene.obstacles)
    return o


_KEPT = {}


def _kept(oracle_mod, key):
    """the samples of a scene the oracle scores as valid (validity does not depend on the weights)"""
    if key not in _KEPT:
        scene = _scene(key)
        o = _oracle(oracle_mod, scene)
        _KEPT[key] = [s for s in SAMPLES if o.score_one(scene.robot_state, s[0], 0.0, s[1], scene.goal_args)[0] >= 0]
        o.close()
    assert len(_KEPT[key]) >= 2, (key, _KEPT[key])
    return _KEPT[key]


def _same_crowd(a, b):
    return (_same(a["cost"], b["cost"]) and a["n_steps"] == b["n_steps"] and _same(a["state"], b["state"]) and
            _same(a["work"], b["work"]) and np.array_equal(a["has_goal"], b["has_goal"]))


def _check_shapes(d, A):
    n = d["n_steps"]
    assert d["state"].shape == (n, A, 4) and d["work"].shape == (n, A) and d["has_goal"].shape == (n, A)
    assert np.all(np.isfinite(d["state"])) and np.all(d["work"] >= 0) and np.all(d["has_goal"][:, 0] == 0)
    assert set(np.unique(d["has_goal"])) <= {0, 1}


# ---- 1. bitwise identities ---------------------------------------------------------------------------------------------------
def test_every_scene_keeps_two_samples_and_the_dense_one_ends_in_a_contact(oracle_mod):
    for key in SCENE_KEYS:
        _kept(oracle_mod, key)
    assert (0.7, 0.0) not in _kept(oracle_mod, (69, 16, 0))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("key", SCENE_KEYS, ids=str)
def test_cost_count_and_robot_row_are_score_ones(oracle_mod, hip_mod, key, precision):
    scene = _scene(key)
    A = len(scene.agents)
    g = _scorer(hip_mod, scene, precision)
    for vx, vth in _kept(oracle_mod, key):
        cost, pts = g.score_one(scene.robot_state, vx, 0.0, vth, scene.goal_args)
        d = g.score_one_crowd(scene.robot_state, vx, 0.0, vth, scene.goal_args)
        _check_shapes(d, A)
        assert _same(d["cost"], cost) and cost >= 0
        n = d["n_steps"]
        assert n == len(pts) == S
        assert _same(d["state"][: n - 1, 0, 0:2], pts[1:n, 0:2])
    g.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_contact_sample_of_the_dense_scene(oracle_mod, hip_mod, precision):
    """(0.7, 0) among 69 people ends in a contact: cost, count and robot row still are sfw_score_one's"""
    scene = _scene((69, 16, 0))
    g = _scorer(hip_mod, scene, precision)
    cost, pts = g.score_one(scene.robot_state, 0.7, 0.0, 0.0, scene.goal_args)
    d = g.score_one_crowd(scene.robot_state, 0.7, 0.0, 0.0, scene.goal_args)
    _check_shapes(d, len(scene.agents))
    n = d["n_steps"]
    assert cost == -1.0 and _same(d["cost"], cost) and 0 < n == len(pts) < S
    assert _same(d["state"][: n - 1, 0, 0:2], pts[1:n, 0:2])
    g.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_grid_crowd_is_score_one_crowd_of_the_sample(hip_mod, precision):
    """the reference's 5 x 9 grid: every sample (the winner and the skipped one among them), and the launch stays as it was"""
    scene = _scene((5, 12, 0))
    lin, ang = syn.reference_sampler()
    g, g1 = _scorer(hip_mod, scene, precision), _scorer(hip_mod, scene, precision)
    g.set_terms_capture(True)
    costs, best = g.score_grid(scene.robot_state, lin, ang, scene.goal_args)
    costs = costs.copy()
    w2 = [[1.0, 1.0, 0.7, 2.0, 1.2], [0.5, 2.0, 0.1, 1.0, 3.0]]
    re_best, re_costs = g.rescore(w2, want_costs=True)
    assert best["index"] >= 0
    for t in range(len(lin) * len(ang)):
        d = g.grid_crowd(t)
        if lin[t // len(ang)] == 0.0 and ang[t % len(ang)] == 0.0:
            assert d["n_steps"] == 0 and d["cost"] == SFW_COST_SKIPPED and d["state"].shape == (0, len(scene.agents), 4)
            continue
        ref = g1.score_one_crowd(scene.robot_state, lin[t // len(ang)], 0.0, ang[t % len(ang)], scene.goal_args)
        assert _same_crowd(d, ref), t
        assert _same(d["cost"], costs[t])
        pts = g.grid_points(t)
        assert d["n_steps"] == len(pts)
    # read-only for the launch
    assert _same(g.costs_view(), costs)
    c2, b2, _ = g.fetch()
    assert _same(c2, costs) and b2 == best
    rb, rc = g.rescore(w2, want_costs=True)
    assert rb == re_best and _same(rc, re_costs)
    # between stage and launch
    g.stage(scene.robot_state, lin, ang, scene.goal_args)
    d0 = g.grid_crowd(best["index"])
    g.launch()
    c3, b3, _ = g.fetch()
    assert _same(c3, costs) and b3 == best and _same_crowd(d0, g.grid_crowd(best["index"]))
    g.close()
    g1.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_grid_crowd_of_a_holonomic_list(hip_mod, precision):
    scene = _scene((20, 14, 16))
    vx = np.array([0.5, 0.1, 0.7, 0.3, 0.0, 0.6])
    vy = np.array([0.2, -0.3, 0.1, 0.25, 0.15, -0.05])
    vth = np.array([0.2, -0.4, 0.0, 0.5, 0.1, -0.2])
    g, g1 = _scorer(hip_mod, scene, precision), _scorer(hip_mod, scene, precision)
    costs, best = g.score_samples(scene.robot_state, vx, vth, HOLO_GA, vy=vy)
    for t in range(6):
        d = g.grid_crowd(t)
        ref = g1.score_one_crowd(scene.robot_state, vx[t], vy[t], vth[t], HOLO_GA)
        assert _same_crowd(d, ref), t
        assert _same(d["cost"], costs[t])
        if d["n_steps"] > 1:
            assert np.any(d["state"][:, 0, 3] != 0.0)  # the robot-local twist has its vy
    assert _same(g.costs_view(), costs)
    g.close()
    g1.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_grid_crowd_of_batch_and_ensemble_members(hip_mod, precision):
    lin, ang = syn.reference_sampler()
    scenes = [_scene((5, 12, 0)), _scene((20, 14, 16))]
    b = hip_mod.BatchScorer(_params(precision), B=2)
    for i, sc in enumerate(scenes):
        b.member(i).load_scene(sc)
        b.stage(i, sc.robot_state, lin, ang, sc.goal_args)
    b.launch()
    bests = b.fetch()
    for i, sc in enumerate(scenes):
        t = bests[i]["index"]
        assert t >= 0
        g1 = _scorer(hip_mod, sc, precision)
        ref = g1.score_one_crowd(sc.robot_state, lin[t // len(ang)], 0.0, ang[t % len(ang)], sc.goal_args)
        assert _same_crowd(b.member(i).grid_crowd(t), ref), i
        assert _same(ref["cost"], b.member(i).costs_view()[t])
        g1.close()
    b.close()
    base, other = _scene((5, 12, 0)), _scene((5, 19, 0))
    e = hip_mod.EnsembleScorer(_params(precision), M=2)
    e.load_scene(base, [base.agents, other.agents])
    costs, rejected, best = e.score_grid(base.robot_state, lin, ang, base.goal_args)
    t = best["index"]
    assert t >= 0
    for m, sc in enumerate((base, other)):
        g1 = _scorer(hip_mod, base, precision)
        g1.set_agents(sc.agents, base.obstacles)
        ref = g1.score_one_crowd(base.robot_state, lin[t // len(ang)], 0.0, ang[t % len(ang)], base.goal_args)
        assert _same_crowd(e.member(m).grid_crowd(t), ref), m
        g1.close()
    c2, r2, b2 = e.aggregate()
    assert _same(c2, costs) and np.array_equal(r2, rejected) and b2 == best  # the members' launches stay as they were
    e.close()


# ---- 2. the work adds up --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("key", SCENE_KEYS, ids=str)
def test_work_sums_to_the_social_term(oracle_mod, hip_mod, key, precision):
    """The bound is the rounding of two summation orders of the same non-negative addends.  An entry IS the addend but for a
    person's work below 1e-140 (f64 modes) / 1e-12 (SFW_PRECISION_F32), which the capture evaluates again in double
    (small_wp, sfw_kernels.hip; test_work_entries_against_pair_force holds every entry with no floor).  Such an entry exceeds
    its addend by what the scoring norm q * rsqrt(q + tiny) lost: at most 0.3 sqrt(tiny) = 3e-151 / 3e-16 each.  In the f64
    modes that is nothing next to any social work; in SFW_PRECISION_F32 the sum moves by at most (replaced entries) x 3e-16
    absolute, which the rounding bound covers for a social work of at least (replaced / (A S)) x 1.4 — not a theorem for a
    scene whose whole social work is of the order of the entries no sum can tell.  The bound is not widened for it; each
    case prints its figure (closest here: 5 people, SFW_PRECISION_F32, sample (0.7, 0): 15 replaced entries move a social
    work of 0.041 by 1.3e-15, 3.2e-14 relative against 4.3e-14)."""
    scene = _scene(key)
    A = len(scene.agents)
    g = _scorer(hip_mod, scene, precision, **SOCIAL_ONLY)
    for vx, vth in _kept(oracle_mod, key):
        d = g.score_one_crowd(scene.robot_state, vx, 0.0, vth, scene.goal_args)
        total = float(np.sum(d["work"]))
        print(f"{key} {vx, vth} prec {precision}: social {d['cost']!r} sum {total!r} rel {abs(total - d['cost']) / d['cost']:.3e}")
        assert d["n_steps"] == S and d["cost"] > 0
        assert abs(total - d["cost"]) <= 2.0 * A * S * 2.0 ** -53 * d["cost"]
    g.close()


# ---- 3. continuation through the oracle -------------------------------------------------------------------------------------
def _agents_from_row(scene, state_row, has_goal_row):
    A = len(scene.agents)
    out = (SfwAgent * A)()
    for a in range(A):
        C.memmove(C.byref(out[a]), C.byref(scene.agents[a]), C.sizeof(SfwAgent))
        out[a].x, out[a].y, out[a].vx, out[a].vy = (float(v) for v in state_row[a])
        out[a].has_goal = int(has_goal_row[a]) if a > 0 else 0
    return out


_ORACLE_W = {}


def _oracle_social(oracle_mod, key, sample, sim_time):
    if (key, sample, sim_time) not in _ORACLE_W:
        scene = _scene(key)
        o = _oracle(oracle_mod, scene, sim_time=sim_time, **SOCIAL_ONLY)
        _ORACLE_W[(key, sample, sim_time)] = o.score_one(scene.robot_state, sample[0], 0.0, sample[1], scene.goal_args)[0]
        o.close()
    return _ORACLE_W[(key, sample, sim_time)]


@pytest.mark.parametrize("precision", F64_MODES)
@pytest.mark.parametrize("key", SCENE_KEYS, ids=str)
def test_oracle_continues_from_a_captured_row(oracle_mod, hip_mod, key, precision):
    k = 12
    scene = _scene(key)
    g = _scorer(hip_mod, scene, precision, **SOCIAL_ONLY)
    for sample in _kept(oracle_mod, key):
        vx, vth = sample
        w_s = _oracle_social(oracle_mod, key, sample, 1.0)
        w_k = _oracle_social(oracle_mod, key, sample, 0.375)
        _, pts = g.score_one(scene.robot_state, vx, 0.0, vth, scene.goal_args)
        d = g.score_one_crowd(scene.robot_state, vx, 0.0, vth, scene.goal_args)
        assert d["n_steps"] == S and len(pts) == S
        vtheta = scene.robot_state[5]
        for _ in range(k):
            vtheta = _new_velocity(vth, vtheta, scene.goal_args[2], DT)
        rs = (pts[k, 0], pts[k, 1], pts[k, 2], d["state"][k - 1, 0, 2], d["state"][k - 1, 0, 3], vtheta)
        o = _oracle(oracle_mod, scene, agents=_agents_from_row(scene, d["state"][k - 1], d["has_goal"][k - 1]), sim_time=0.625,
                    **SOCIAL_ONLY)
        w_rest = o.score_one(rs, vx, 0.0, vth, scene.goal_args)[0]
        o.close()
        print(f"{key} {sample} prec {precision}: W_S {w_s!r} W_k {w_k!r} W' {w_rest!r} rel {abs(w_k + w_rest - w_s) / w_s:.3e}")
        assert w_s > 0 and w_k > 0 and w_rest > 0
        assert abs(w_k + w_rest - w_s) <= RTOL_F64 * w_s
    g.close()


# ---- 4. per-entry work against the oracle's pair force ------------------------------------------------------------------------
def _agent(x, y, vx, vy):
    a = SfwAgent()
    a.x, a.y, a.vx, a.vy = float(x), float(y), float(vx), float(vy)
    return a


_ENTRIES = {}


def _entries(oracle_mod, hip_mod, key, precision):
    """Every work entry of a scene's kept samples next to its reference, computed once per (scene, precision):
    person entries work[i, a] against |pair_force(person a of row i, robot of row i)|, robot entries work[i, 0] against
    |sum_j pair_force(robot of row i - 1, person j of row i - 1)| (i = 0: the handed-over agents) with the sum of the |f_j|."""
    if (key, precision) in _ENTRIES:
        return _ENTRIES[(key, precision)]
    scene = _scene(key)
    A = len(scene.agents)
    p = _params()
    g = _scorer(hip_mod, scene, precision)
    start = np.array([[a.x, a.y, a.vx, a.vy] for a in scene.agents])
    samples = _kept(oracle_mod, key)
    dev_p, ref_p = np.zeros((len(samples), S, A - 1)), np.zeros((len(samples), S, A - 1))
    dev_r, ref_r, abs_r = np.zeros((len(samples), S)), np.zeros((len(samples), S)), np.zeros((len(samples), S))
    for n, (vx, vth) in enumerate(samples):
        d = g.score_one_crowd(scene.robot_state, vx, 0.0, vth, scene.goal_args)
        assert d["n_steps"] == S
        dev_p[n], dev_r[n] = d["work"][:, 1:], d["work"][:, 0]
        for i in range(S):
            row, prev = d["state"][i], (d["state"][i - 1] if i > 0 else start)
            robot, robot_prev = _agent(*row[0]), _agent(*prev[0])
            fsum = np.zeros(2)
            for a in range(1, A):
                f = oracle_mod.pair_force(p, _agent(*row[a]), robot)
                ref_p[n, i, a - 1] = np.hypot(f[0], f[1])
                f = oracle_mod.pair_force(p, robot_prev, _agent(*prev[a]))
                fsum += f
                abs_r[n, i] += np.hypot(f[0], f[1])
            ref_r[n, i] = np.hypot(fsum[0], fsum[1])
    g.close()
    _ENTRIES[(key, precision)] = (dev_p, ref_p, dev_r, ref_r, abs_r)
    return _ENTRIES[(key, precision)]


def _entry_rtol(precision):
    return RTOL_NORTH_STAR if precision == SFW_PRECISION_F32 else RTOL_F64


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("key", PLAIN_KEYS, ids=str)
def test_work_entries_against_pair_force(oracle_mod, hip_mod, key, precision):
    """Every entry, relative, with no floor.  A Wp far below anything a sum can tell (down to 1e-171 at 69 people) is held
    like any other: the scoring pass's norm q * rsqrt(q + tiny) would come out low there (and 0 once q underflows), so the
    capture evaluates such an entry again in double with a scaled norm (small_wp, sfw_kernels.hip)."""
    rtol = _entry_rtol(precision)
    dev_p, ref_p, dev_r, ref_r, abs_r = _entries(oracle_mod, hip_mod, key, precision)
    bad_p = np.abs(dev_p - ref_p) > rtol * ref_p
    print(f"{key} prec {precision}: worst person entry {np.max(np.abs(dev_p - ref_p) / ref_p):.3e}, worst robot entry "
          f"{np.max(np.abs(dev_r - ref_r) / abs_r):.3e} (of the summed magnitudes); {int(bad_p.sum())} person entries beyond "
          f"{rtol:g}" + (f", the largest reference among them {ref_p[bad_p].max():.3e}" if bad_p.any() else ""))
    assert np.all(np.abs(dev_r - ref_r) <= rtol * abs_r)
    assert not bad_p.any(), (int(bad_p.sum()), float(ref_p[bad_p].max()), dev_p[bad_p][:3], ref_p[bad_p][:3])


# ---- 5. integrator consistency from the rows alone ------------------------------------------------------------------------------
def _goal_scene():
    """(5, 12, 0) with person 1 walking at 0.8 m/s towards a goal 0.5 m ahead (radius 0.35): reached after about 0.2 s"""
    base = _scene((5, 12, 0))
    agents = (SfwAgent * len(base.agents))()
    for a in range(len(base.agents)):
        C.memmove(C.byref(agents[a]), C.byref(base.agents[a]), C.sizeof(SfwAgent))
    p = agents[1]
    p.x, p.y, p.vx, p.vy = 3.0, 3.0, 0.8, 0.0
    p.goal_x, p.goal_y, p.goal_radius, p.has_goal = 3.5, 3.0, 0.35, 1
    return dataclasses.replace(base, agents=agents)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("key", SCENE_KEYS + ["goal"], ids=str)
def test_rows_follow_the_integrator(oracle_mod, hip_mod, key, precision):
    scene = _goal_scene() if key == "goal" else _scene(key)
    samples = SAMPLES[:2] if key == "goal" else _kept(oracle_mod, key)
    A = len(scene.agents)
    dv = np.array([a.desired_velocity for a in scene.agents])[1:]
    goal = np.array([[a.goal_x, a.goal_y] for a in scene.agents])[1:]
    gr = np.array([a.goal_radius for a in scene.agents])[1:]
    hg0 = np.array([a.has_goal for a in scene.agents])[1:]
    start = np.array([[a.x, a.y] for a in scene.agents])[1:]
    g = _scorer(hip_mod, scene, precision)
    for vx, vth in samples:
        d = g.score_one_crowd(scene.robot_state, vx, 0.0, vth, scene.goal_args)
        n = d["n_steps"]
        assert n == S
        pos, vel, hg = d["state"][:, 1:, 0:2], d["state"][:, 1:, 2:4], d["has_goal"][:, 1:]
        speed = np.hypot(vel[..., 0], vel[..., 1])
        assert np.all(speed <= dv * (1.0 + 2.0 ** -50)), float(np.max(speed / dv))
        prev = np.concatenate([start[None], pos[:-1]])
        step = vel * DT
        resid = np.abs(pos - (prev + step))
        assert np.all(resid <= 2.0 * 2.0 ** -52 * np.maximum(np.abs(pos), np.abs(step))), float(np.max(resid))
        # has_goal never comes back, and drops exactly at the first row inside the goal's radius
        full = np.concatenate([hg0[None], hg])
        assert np.all(full[1:] <= full[:-1])
        dist = np.hypot(goal[None, :, 0] - pos[..., 0], goal[None, :, 1] - pos[..., 1])
        clear = np.all(np.abs(dist - gr) >= 1e-6, axis=0) & (hg0 == 1)  # people whose pop step does not hang on a rounding
        expect = (np.cumsum(dist <= gr, axis=0) == 0).astype(np.int32)
        assert np.array_equal(hg[:, clear], expect[:, clear])
        if key == "goal":
            assert clear[0], float(np.min(np.abs(dist[:, 0] - gr[0])))
            first = int(np.argmax(dist[:, 0] <= gr[0]))
            assert 0 < first < S - 1 and hg[first - 1, 0] == 1 and hg[first, 0] == 0
    assert A == len(scene.agents)
    g.close()


# ---- 6. early ends, caps, argument and state checks ------------------------------------------------------------------------------
def _contact_scene():
    """one slow person standing 0.8 m ahead on the robot's axis"""
    base = _scene((1, 11, 0))
    agents = (SfwAgent * 2)()
    for a in range(2):
        C.memmove(C.byref(agents[a]), C.byref(base.agents[a]), C.sizeof(SfwAgent))
    p = agents[1]
    p.x, p.y, p.vx, p.vy, p.has_goal, p.desired_velocity = 0.8, 0.0, 0.0, 0.0, 0, 0.05
    return dataclasses.replace(base, agents=agents)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_pedestrian_contact_ends_the_rows(oracle_mod, hip_mod, precision):
    scene = _contact_scene()
    o = _oracle(oracle_mod, scene)
    oc, opts = o.score_one(scene.robot_state, 0.7, 0.0, 0.0, scene.goal_args)
    o.close()
    c = len(opts) - 1
    assert oc == -1.0 and 0 < c < S - 1
    g = _scorer(hip_mod, scene, precision)
    d = g.score_one_crowd(scene.robot_state, 0.7, 0.0, 0.0, scene.goal_args)
    assert d["cost"] == -1.0 and d["n_steps"] == c + 1
    rr = float(np.float32(0.35) * np.float32(0.35))  # float-squared, ref :617
    dx, dy = d["state"][:, 0, 0] - d["state"][:, 1, 0], d["state"][:, 0, 1] - d["state"][:, 1, 1]
    touch = dx * dx + dy * dy <= rr
    assert touch[c] and not np.any(touch[:c])
    g.close()


def _lethal_scene():
    """a lethal cell on the x axis 0.3 m ahead, point footprint, the one person far away"""
    base = syn.make_scene(_workload(1, 11, 0, footprint="point"))
    cells = base.cells.copy()
    my, mx = int((0.0 - base.origin_y) / base.resolution), int((0.3 - base.origin_x) / base.resolution)
    cells[my - 1:my + 1, mx:mx + 2] = 254
    agents = (SfwAgent * 2)()
    for a in range(2):
        C.memmove(C.byref(agents[a]), C.byref(base.agents[a]), C.sizeof(SfwAgent))
    p = agents[1]
    p.x, p.y, p.vx, p.vy, p.goal_x, p.goal_y = -3.0, -3.0, -0.5, -0.5, -4.0, -4.0
    return dataclasses.replace(base, cells=cells, agents=agents)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_illegal_footprint_ends_the_rows(oracle_mod, hip_mod, precision):
    scene = _lethal_scene()
    o = _oracle(oracle_mod, scene)
    oc, opts = o.score_one(scene.robot_state, 0.7, 0.0, 0.0, scene.goal_args)
    o.close()
    j = len(opts)
    assert oc == -1.0 and 0 < j < S
    g = _scorer(hip_mod, scene, precision)
    cost, pts = g.score_one(scene.robot_state, 0.7, 0.0, 0.0, scene.goal_args)
    d = g.score_one_crowd(scene.robot_state, 0.7, 0.0, 0.0, scene.goal_args)
    assert d["cost"] == -1.0 == cost and d["n_steps"] == j == len(pts)
    _check_shapes(d, 2)
    assert _same(d["state"][: j - 1, 0, 0:2], pts[1:j, 0:2])
    # ... and as a grid sample
    g.stage(scene.robot_state, [0.7], [0.0], scene.goal_args)
    assert _same_crowd(g.grid_crowd(0), d)
    g.close()


def test_steps_cap_wrong_agent_count_and_state(hip_mod):
    scene = _scene((5, 12, 0))
    A = len(scene.agents)
    L = hip_mod.lib()
    from social_force_window_planner_amd._abi import SfwGoalArgs, SfwRobotState

    rs, ga = SfwRobotState(*scene.robot_state), SfwGoalArgs(*scene.goal_args)
    g = _scorer(hip_mod, scene)
    full = g.score_one_crowd(scene.robot_state, 0.5, 0.0, 0.2, scene.goal_args)
    assert full["n_steps"] == S
    canary = -777.25
    state, work = np.full((S, A, 4), canary), np.full((S, A), canary)
    hg = np.full((S, A), -7, dtype=np.int32)
    cost, n = C.c_double(canary), C.c_int32(-7)

    def call(agents, cap, state_p=state.ctypes.data, n_p=C.byref(n)):
        return L.sfw_score_one_crowd(g._h, C.byref(rs), 0.5, 0.0, 0.2, C.byref(ga), C.byref(cost), state_p, work.ctypes.data,
                                     hg.ctypes.data, agents, cap, n_p)

    # refused before anything is written
    for rc in (call(A + 1, S), call(A - 1, S), call(A, 0), call(A, S, state_p=None), call(A, S, n_p=None)):
        assert rc == SFW_ERR_INVALID_ARG
    assert np.all(state == canary) and np.all(work == canary) and np.all(hg == -7) and n.value == -7 and cost.value == canary
    # steps_cap rows written, the full count reported
    assert call(A, 5) == 0
    assert n.value == S and _same(cost.value, full["cost"])
    assert _same(state[:5], full["state"][:5]) and _same(work[:5], full["work"][:5]) and np.array_equal(hg[:5], full["has_goal"][:5])
    assert np.all(state[5:] == canary) and np.all(work[5:] == canary) and np.all(hg[5:] == -7)
    # work / has_goal are nullable
    n2 = C.c_int32()
    assert L.sfw_score_one_crowd(g._h, C.byref(rs), 0.5, 0.0, 0.2, C.byref(ga), C.byref(cost), state.ctypes.data, None, None, A, S,
                                 C.byref(n2)) == 0
    assert n2.value == S and _same(state, full["state"])
    # the grid call: the same checks, and it needs a stage
    lin, ang = syn.reference_sampler()
    state[:] = canary
    n.value = -7
    assert L.sfw_grid_crowd(g._h, 3, C.byref(cost), state.ctypes.data, None, None, A, S, C.byref(n)) == SFW_ERR_STATE
    g.stage(scene.robot_state, lin, ang, scene.goal_args)
    for rc in (L.sfw_grid_crowd(g._h, 3, C.byref(cost), state.ctypes.data, None, None, A + 1, S, C.byref(n)),
               L.sfw_grid_crowd(g._h, 3, C.byref(cost), state.ctypes.data, None, None, A, 0, C.byref(n)),
               L.sfw_grid_crowd(g._h, 45, C.byref(cost), state.ctypes.data, None, None, A, S, C.byref(n)),
               L.sfw_grid_crowd(g._h, -1, C.byref(cost), state.ctypes.data, None, None, A, S, C.byref(n)),
               L.sfw_grid_crowd(g._h, 3, C.byref(cost), None, None, None, A, S, C.byref(n))):
        assert rc == SFW_ERR_INVALID_ARG
    assert np.all(state == canary) and n.value == -7
    assert L.sfw_grid_crowd(g._h, 3, None, state.ctypes.data, None, None, A, 4, C.byref(n)) == 0  # cost_out is nullable here
    assert n.value == S and np.all(state[4:] == canary) and not np.any(state[:4] == canary)
    # the scalar call consumes the stage, as sfw_score_one does
    assert L.sfw_grid_launch(g._h) == 0
    g.fetch()
    g.stage(scene.robot_state, lin, ang, scene.goal_args)
    g.score_one_crowd(scene.robot_state, 0.5, 0.0, 0.2, scene.goal_args)
    assert L.sfw_grid_launch(g._h) == SFW_ERR_STATE
    assert L.sfw_grid_crowd(g._h, 3, None, state.ctypes.data, None, None, A, S, C.byref(n)) == SFW_ERR_STATE
    g.close()


def test_no_agents_and_robot_alone(hip_mod):
    """0 rows without agents; a robot alone (no pair, no laser point) has rows of zero work"""
    scene = syn.make_scene(_workload(0, 21, 0))
    g = _scorer(hip_mod, scene)
    cost, pts = g.score_one(scene.robot_state, 0.5, 0.0, 0.2, scene.goal_args)
    d = g.score_one_crowd(scene.robot_state, 0.5, 0.0, 0.2, scene.goal_args)
    assert _same(d["cost"], cost) and d["n_steps"] == S == len(pts) and d["state"].shape == (S, 1, 4)
    assert np.all(d["work"] == 0.0) and _same(d["state"][: S - 1, 0, 0:2], pts[1:, 0:2])
    empty = (SfwAgent * 0)()
    g.set_agents(empty, None)
    # (another command than above: a cost left behind by that call would not pass for this one's)
    cost0 = cost
    cost, _ = g.score_one(scene.robot_state, 0.1, 0.0, -0.4, scene.goal_args)
    d = g.score_one_crowd(scene.robot_state, 0.1, 0.0, -0.4, scene.goal_args)
    assert not _same(cost, cost0)
    assert _same(d["cost"], cost) and d["n_steps"] == 0 and d["state"].shape == (0, 0, 4)
    g.close()
