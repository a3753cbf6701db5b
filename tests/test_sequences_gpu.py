"""Command sequences (sfw_sequences_stage / sfw_score_sequences): samples whose command changes inside the horizon.

What is held to what (the contract points of include/sfw_hip.h):
  1. K = 1 is the sample list, bit for bit (costs, best, terms, points, crowd), on the one-launch kernel and without it;
  2. constant sequences equal the list, whatever the knot steps are;
  3. knots at or past the step count are ignored;
  4. causality: what a later knot changes starts at its step;
  5. a sample's cost does not depend on its place, its neighbours, the one-launch kernel, the chunking or the K1 kernel;
  6. selection over the FIRST knot, index_base, n_valid, re-score;
  7. the CPU oracle, through continuation: the oracle scores the first segment from the start and the second from the world
     the existing calls captured after 12 steps of the first; every term of the sequence sample is held to their combination;
  8. early ends (illegal footprint, pedestrian contact) inside the second segment;
  9. refusals, the stage state machine, batches;
 10. a pinned person: standing until a knot is reproduced, braking to rest behind a knot is flagged.
"Bitwise" compares uint64 views.  Every scene is one wave of S = 32 steps with dt = 2^-5 exactly (12 + 20 steps are
sim_time 0.375 + 0.625), the synthetic scenes of tests/test_crowd_gpu.py."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from social_force_window_planner_amd import synthetic as syn
from social_force_window_planner_amd._abi import (SFW_COST_INVALID, SFW_COST_SKIPPED, SFW_ERR_INVALID_ARG, SFW_ERR_STATE,
                                                   SFW_PRECISION_F32, SFW_PRECISION_F64, SFW_PRECISION_F64_STRICT, SfwAgent)
from sfw_test_util import _bits, _commands, _group_scene as _scene, _new_velocity, _np_best, _params, _same, _scorer, _workload

pytestmark = pytest.mark.gpu

RTOL_F64 = 1e-9  # the project's parity tolerance (tests/test_parity_gpu.py)
GRAN = 0.03125
S = 32
DT = 2.0 ** -5
KNOT = 12  # the step at which the second knot of a two-knot sequence takes over
PRECISIONS = [SFW_PRECISION_F64, SFW_PRECISION_F64_STRICT, SFW_PRECISION_F32]
F64_MODES = [SFW_PRECISION_F64, SFW_PRECISION_F64_STRICT]
# (people, seed, laser points): 5, 20 and 40 people, 20 people with 16 laser points, "group": 8 people, five in two groups
SCENE_KEYS = [(5, 12, 0), (20, 13, 0), (20, 14, 16), (40, 15, 0), "group"]
SAMPLES = [(0.5, 0.2), (0.1, -0.4), (0.7, 0.0)]  # (vx, vtheta), as tests/test_crowd_gpu.py
PAIRS = [(c1, c2) for c1 in SAMPLES for c2 in SAMPLES if c1 != c2]
SOCIAL_ONLY = dict(vel_weight=0.0, distance_weight=0.0, angle_weight=0.0, costmap_weight=0.0, social_weight=1.0)
WEIGHT_NAMES = ("vel_weight", "distance_weight", "angle_weight", "costmap_weight", "social_weight")  # SFW_TERM_* order
T_VEL, T_DIST, T_ANG, T_CM, T_SOC = range(5)
HOLO_GA = (1.0, 0.7, 1.0, 2.0, 0.5)


# ---- the scenes and helpers of tests/test_crowd_gpu.py ----------------------------------------------------------------------------
def _oracle(oracle_mod, scene, agents=None, sim_time=1.0, **kw):
    o = oracle_mod.OracleScorer(_params(sim_time=sim_time, **kw))
    o.set_costmap(scene.cells, scene.origin_x, scene.origin_y, scene.resolution)
    o.set_footprint(scene.footprint)
    o.set_agents(scene.agents if agents is None else agents, scene.obstacles)
    return o


def _same_crowd(a, b):
    return (_same(a["cost"], b["cost"]) and a["n_steps"] == b["n_steps"] and _same(a["state"], b["state"]) and
            _same(a["work"], b["work"]) and np.array_equal(a["has_goal"], b["has_goal"]))


def _agents_from_row(scene, state_row, has_goal_row):
    A = len(scene.agents)
    out = (SfwAgent * A)()
    for a in range(A):
        C.memmove(C.byref(out[a]), C.byref(scene.agents[a]), C.sizeof(SfwAgent))
        out[a].x, out[a].y, out[a].vx, out[a].vy = (float(v) for v in state_row[a])
        out[a].has_goal = int(has_goal_row[a]) if a > 0 else 0
    return out


def _copy_agents(scene):
    agents = (SfwAgent * len(scene.agents))()
    for a in range(len(scene.agents)):
        C.memmove(C.byref(agents[a]), C.byref(scene.agents[a]), C.sizeof(SfwAgent))
    return agents


# ---- sequences -------------------------------------------------------------------------------------------------------------------
def _two_knots(pairs):
    """(2, n) vx and vtheta of the two-knot sequences (c1 until KNOT, c2 after)"""
    vx = np.array([[c1[0] for c1, _ in pairs], [c2[0] for _, c2 in pairs]])
    vth = np.array([[c1[1] for c1, _ in pairs], [c2[1] for _, c2 in pairs]])
    return vx, vth


def _no_skip_no_nan(costs):
    return not np.any(np.isnan(costs)) and not np.any(costs == SFW_COST_SKIPPED)


# ---- 1. K = 1 is the list ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_knot_is_the_sample_list(hip_mod, monkeypatch, precision, fused):
    monkeypatch.setenv("SFW_CYCLE_FUSED", "1" if fused else "0")
    scene = _scene((20, 14, 16))
    vx, vy, vth = _commands(9, 31)
    gl, gs = _scorer(hip_mod, scene, precision), _scorer(hip_mod, scene, precision)
    gl.set_terms_capture(True)
    gs.set_terms_capture(True)
    lc, lb = gl.score_samples(scene.robot_state, vx[0], vth[0], HOLO_GA, vy=vy[0])
    gs.stage_sequences(scene.robot_state, vx, vth, [0], HOLO_GA, vy=vy)
    plan = gs.plan_info()
    assert (fused or plan["one_launch"] == 0) and plan["levels"] == 0 and plan["samples"] == 9, plan
    gs.launch()
    sc, sb, _ = gs.fetch()
    assert _same(sc, lc) and sb == lb and _no_skip_no_nan(sc)
    assert _same(gs.cost_terms(), gl.cost_terms())
    lp, ln = gl.grid_points_batch(0, 9, S)
    sp, sn = gs.grid_points_batch(0, 9, S)
    assert np.array_equal(ln, sn) and _same(lp, sp)
    for t in (2, 7):
        assert _same_crowd(gs.grid_crowd(t), gl.grid_crowd(t)), t
    # no vy at all is the list without one
    lc0, lb0 = gl.score_samples(scene.robot_state, vx[0], vth[0], HOLO_GA)
    sc0, sb0 = gs.score_sequences(scene.robot_state, vx, vth, [0], HOLO_GA)
    assert _same(sc0, lc0) and sb0 == lb0
    gl.close()
    gs.close()


# ---- 2. constant sequences -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [(0, 7, 19), tuple(range(64))], ids=["K3", "K64"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_constant_sequences_equal_the_list(hip_mod, precision, steps):
    scene = _scene((20, 13, 0))
    K = len(steps)
    vx, vy, vth = _commands(45, 32)
    g = _scorer(hip_mod, scene, precision)
    g.set_terms_capture(True)
    lc, lb = g.score_samples(scene.robot_state, vx[0], vth[0], HOLO_GA, vy=vy[0])
    lt = g.cost_terms()
    sc, sb = g.score_sequences(scene.robot_state, np.tile(vx, (K, 1)), np.tile(vth, (K, 1)), steps, HOLO_GA, vy=np.tile(vy, (K, 1)))
    assert _same(sc, lc) and sb == lb and _same(g.cost_terms(), lt) and _no_skip_no_nan(sc)
    assert np.sum(sc >= 0) >= 2
    g.close()


# ---- 3. knots at or past the step count ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_knots_at_or_past_the_horizon_are_ignored(hip_mod, precision):
    scene = _scene((5, 12, 0))
    vx, vy, vth = _commands(45, 33, K=3)
    g = _scorer(hip_mod, scene, precision)
    g.set_terms_capture(True)
    g.stage_sequences(scene.robot_state, vx[:2], vth[:2], (0, 12), HOLO_GA, vy=vy[:2])
    assert g.plan_info()["one_launch"] == 1  # (5 people, 45 samples: the one-launch kernel's home case)
    g.launch()
    c2, b2, _ = g.fetch()
    c2 = c2.copy()
    t2 = g.cost_terms()
    held, _ = g.score_samples(scene.robot_state, vx[0], vth[0], HOLO_GA, vy=vy[0])
    assert not _same(c2, held)  # (the second knot matters ...)
    for steps in ((0, 12, 32), (0, 12, 40)):  # (... the third, never reached, does not)
        c3, b3 = g.score_sequences(scene.robot_state, vx, vth, steps, HOLO_GA, vy=vy)
        assert _same(c3, c2) and b3 == b2 and _same(g.cost_terms(), t2), steps
    c31, b31 = g.score_sequences(scene.robot_state, vx, vth, (0, 12, 31), HOLO_GA, vy=vy)
    assert not _same(c31, c2)  # (a knot at the last step is reached: the velocity term reads that step's vx)
    g.close()


# ---- 4. causality ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(5, 12, 0), "group"], ids=str)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_later_knot_changes_nothing_before_its_step(hip_mod, precision, key):
    scene = _scene(key)
    n = len(PAIRS)
    vx, vth = _two_knots(PAIRS + [(c1, c1) for c1, _ in PAIRS])  # sample n + t: c1 held
    g = _scorer(hip_mod, scene, precision)
    g.stage_sequences(scene.robot_state, vx, vth, (0, KNOT), scene.goal_args)
    pts, npts = g.grid_points_batch(0, 2 * n, S)
    for t in range(n):
        a, b = g.grid_crowd(t), g.grid_crowd(n + t)
        assert npts[t] > KNOT + 1 and npts[n + t] > KNOT + 1 and a["n_steps"] > KNOT and b["n_steps"] > KNOT, (t, npts[t], npts[n + t])
        assert _same(pts[t, :KNOT + 1], pts[n + t, :KNOT + 1]), t
        assert _same(a["state"][:KNOT], b["state"][:KNOT]) and _same(a["work"][:KNOT], b["work"][:KNOT]), t
        assert np.array_equal(a["has_goal"][:KNOT], b["has_goal"][:KNOT])
        assert not _same(pts[t, KNOT + 1], pts[n + t, KNOT + 1]), t  # the pose after step KNOT
        assert not _same(a["state"][KNOT, 0], b["state"][KNOT, 0]), t
    g.close()


# ---- 5. placement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_cost_does_not_depend_on_placement_kernel_or_chunking(hip_mod, monkeypatch, precision):
    scene = _scene((20, 14, 16))
    steps = (0, 7, 19)
    vx, vy, vth = _commands(45, 34, K=3)
    rs = scene.robot_state
    g = _scorer(hip_mod, scene, precision)
    g.stage_sequences(rs, vx, vth, steps, HOLO_GA, vy=vy)
    g.launch()
    ref, rb, _ = g.fetch()
    ref = ref.copy()
    assert _no_skip_no_nan(ref) and np.sum(ref >= 0) >= 2 and rb == _np_best(ref, vx[0], vy[0], vth[0])
    # permuted, with duplicates
    perm = np.random.default_rng(5).permutation(45)
    perm = np.concatenate([perm, perm[[3, 11, 17, 29, 40]]])
    c, b = g.score_sequences(rs, vx[:, perm], vth[:, perm], steps, HOLO_GA, vy=vy[:, perm])
    assert _same(c, ref[perm]) and b == _np_best(c, vx[0, perm], vy[0, perm], vth[0, perm])
    # each sample alone
    for t in range(45):
        c, _ = g.score_sequences(rs, vx[:, t:t + 1], vth[:, t:t + 1], steps, HOLO_GA, vy=vy[:, t:t + 1])
        assert _same(c, ref[t:t + 1]), t
    # without the one-launch kernel: the small-grid K1
    monkeypatch.setenv("SFW_CYCLE_FUSED", "0")
    g.stage_sequences(rs, vx, vth, steps, HOLO_GA, vy=vy)
    assert g.plan_info()["one_launch"] == 0
    g.launch()
    c, b, _ = g.fetch()
    assert _same(c, ref) and b == rb
    monkeypatch.delenv("SFW_CYCLE_FUSED")
    # embedded in 2100 samples: the team K1 and the thread K1
    bx, by, bth = _commands(2100, 35, K=3)
    pos = np.sort(np.random.default_rng(6).choice(2100, 45, replace=False))
    bx[:, pos], by[:, pos], bth[:, pos] = vx, vy, vth
    big = []
    for threads in ("0", "1"):
        monkeypatch.setenv("SFW_K1A_THREADS", threads)
        g.stage_sequences(rs, bx, bth, steps, HOLO_GA, vy=by)
        plan = g.plan_info()
        assert plan["one_launch"] == 0 and plan["chunks"] == 1 and plan["samples"] == 2100 and plan["levels"] == 0, plan
        g.launch()
        c, b, _ = g.fetch()
        assert _same(c[pos], ref), (threads, np.flatnonzero(_bits(c[pos]) != _bits(ref)))
        assert b == _np_best(c, bx[0], by[0], bth[0]) and _no_skip_no_nan(c)
        big.append(c.copy())
    monkeypatch.delenv("SFW_K1A_THREADS")
    assert _same(big[0], big[1])
    # ... and chunked (chunk floor 1024 < 2100)
    monkeypatch.setenv("SFW_TABLE_BUDGET_MB", "1")
    g2 = _scorer(hip_mod, scene, precision)
    g2.stage_sequences(rs, bx, bth, steps, HOLO_GA, vy=by)
    assert g2.plan_info()["chunks"] > 1
    g2.launch()
    c, b, _ = g2.fetch()
    assert _same(c, big[0]) and _same(c[pos], ref)
    # a dump of a sample of the second chunk hands K1 that sample's knots
    t = int(pos[-1])
    assert t >= 1024
    p_big = g2.grid_points(t)
    g.stage_sequences(rs, vx, vth, steps, HOLO_GA, vy=vy)
    assert _same(p_big, g.grid_points(44))
    g.close()
    g2.close()


# ---- 6. selection ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_selection_reads_the_first_knot(hip_mod, precision):
    scene = _scene((40, 15, 0))
    steps = (0, 12)
    vx, vy, vth = _commands(40, 36, K=2)
    g = _scorer(hip_mod, scene, precision)
    g.set_terms_capture(True)
    costs, best = g.score_sequences(scene.robot_state, vx, vth, steps, HOLO_GA, vy=vy)
    w = best["index"]
    assert 0 <= w < 40 and best == _np_best(costs, vx[0], vy[0], vth[0])
    assert best["n_valid"] == int(np.sum(costs >= 0)) >= 1
    assert (best["vx"], best["vy"], best["vtheta"]) == (vx[0, w], vy[0, w], vth[0, w])  # the first knot's three values
    # re-score of the captured terms is score_sequences under those weights, field for field
    weights = [(1.0, 1.0, 0.7, 2.0, 1.2), (0.2, 3.0, 0.0, 0.5, 4.0), (2.0, 0.5, -0.3, 1.0, 0.1)]
    bests, rc = g.rescore(weights, want_costs=True)
    for k, wv in enumerate(weights):
        f = _scorer(hip_mod, scene, precision, **dict(zip(WEIGHT_NAMES, wv)))
        fc, fb = f.score_sequences(scene.robot_state, vx, vth, steps, HOLO_GA, vy=vy)
        assert _same(rc[k], fc) and bests[k] == fb, (k, bests[k], fb)
        f.close()
    # an exact copy of the winner appended wins by its index
    ax, ay, ath = (np.concatenate([a, a[:, w:w + 1]], axis=1) for a in (vx, vy, vth))
    c2, b2 = g.score_sequences(scene.robot_state, ax, ath, steps, HOLO_GA, vy=ay)
    assert _same(c2[:40], costs) and _same(c2[40], costs[w])
    assert b2["index"] == 40 and b2["cost"] == best["cost"] and b2["n_valid"] == best["n_valid"] + 1
    # index_base enters the key
    g.stage_sequences(scene.robot_state, vx, vth, steps, HOLO_GA, vy=vy, index_base=1000)
    g.launch()
    c3, b3, key = g.fetch()
    assert _same(c3, costs) and b3 == best
    assert key == (best["cost"], -vx[0, w], abs(vth[0, w]), float(-(1000 + w)))
    g.close()


# ---- 7. the oracle, through continuation ----------------------------------------------------------------------------------------------
def _oracle_terms(oracle_mod, scene, agents, rs, cmd, sim_time, ga=None):
    """(valid, the five unweighted terms, Trajectory points) of one constant command by the CPU oracle: one weight at 1 and
    the rest at 0 per term, as SOCIAL_ONLY does"""
    terms, pts = [], None
    for name in WEIGHT_NAMES:
        o = _oracle(oracle_mod, scene, agents=agents, sim_time=sim_time, **{n: (1.0 if n == name else 0.0) for n in WEIGHT_NAMES})
        c, pts = o.score_one(rs, cmd[0], 0.0, cmd[1], scene.goal_args if ga is None else ga)
        o.close()
        terms.append(c)
    valid = all(c >= 0 for c in terms)
    assert valid or all(c == -1.0 for c in terms), terms
    return valid, terms, pts


def _continuation(g, scene, c1, ga=None, k=KNOT):
    """The world after k steps of the constant command c1, from the EXISTING calls (sfw_score_one / sfw_score_one_crowd, held
    to the oracle by tests/test_crowd_gpu.py): the robot state and agents that test_oracle_continues_from_a_captured_row builds"""
    ga = scene.goal_args if ga is None else ga
    _, pts = g.score_one(scene.robot_state, c1[0], 0.0, c1[1], ga)
    d = g.score_one_crowd(scene.robot_state, c1[0], 0.0, c1[1], ga)
    assert d["n_steps"] >= k and len(pts) > k, (d["n_steps"], len(pts))
    vtheta = scene.robot_state[5]
    for _ in range(k):
        vtheta = _new_velocity(c1[1], vtheta, ga[2], DT)
    rs = (pts[k, 0], pts[k, 1], pts[k, 2], d["state"][k - 1, 0, 2], d["state"][k - 1, 0, 3], vtheta)
    return rs, _agents_from_row(scene, d["state"][k - 1], d["has_goal"][k - 1])


def _close(got, want):
    return abs(got - want) <= (RTOL_F64 * abs(want) if want != 0.0 else RTOL_F64)


_FIRST_HALF = {}


def _first_half(oracle_mod, key, c1):
    if (key, c1) not in _FIRST_HALF:
        scene = _scene(key)
        _FIRST_HALF[(key, c1)] = _oracle_terms(oracle_mod, scene, None, scene.robot_state, c1, 0.375)
    return _FIRST_HALF[(key, c1)]


@pytest.mark.parametrize("precision", F64_MODES)
@pytest.mark.parametrize("key", SCENE_KEYS, ids=str)
def test_oracle_scores_the_two_segments(oracle_mod, hip_mod, key, precision):
    """Sequence (c1 until step 12, c2 after) for every ordered pair of SAMPLES with c1 != c2.  The oracle (oracle/ as it stands)
    scores c1 from the start over sim_time 0.375 and c2 over 0.625 from the world after 12 steps of c1; a pair counts when it
    finds both halves valid, and at least two pairs per scene must count.  Per term, RTOL_F64 relative (absolute for a term
    that is 0): social = W12(c1) + W'(c2); costmap = (12 cm1 + 20 cm2) / 32; distance, angle and velocity = the
    continuation's; points 13..31 = the continuation's."""
    scene = _scene(key)
    vx, vth = _two_knots(PAIRS)
    g, g1 = _scorer(hip_mod, scene, precision), _scorer(hip_mod, scene, precision)
    g.set_terms_capture(True)
    costs, _ = g.score_sequences(scene.robot_state, vx, vth, (0, KNOT), scene.goal_args)
    terms = g.cost_terms()
    pts, npts = g.grid_points_batch(0, len(PAIRS), S)
    conts = {c1: _continuation(g1, scene, c1) for c1 in SAMPLES}
    counted = 0
    for t, (c1, c2) in enumerate(PAIRS):
        ok1, t1, _ = _first_half(oracle_mod, key, c1)
        rs_k, agents_k = conts[c1]
        ok2, t2, opts = _oracle_terms(oracle_mod, scene, agents_k, rs_k, c2, 0.625)
        print(f"{key} {c1}->{c2} prec {precision}: halves valid {ok1, ok2}, cost {costs[t]!r}")
        if not (ok1 and ok2):
            assert costs[t] == SFW_COST_INVALID, (t, costs[t])
            continue
        counted += 1
        want = [t2[T_VEL], t2[T_DIST], t2[T_ANG], (12.0 * t1[T_CM] + 20.0 * t2[T_CM]) / 32.0, t1[T_SOC] + t2[T_SOC]]
        for k in range(5):
            print(f"    {WEIGHT_NAMES[k]}: {terms[t, k]!r} want {want[k]!r} rel {abs(terms[t, k] - want[k]) / max(abs(want[k]), 1e-300):.3e}")
        assert costs[t] >= 0 and npts[t] == S and len(opts) == S - KNOT
        assert t1[T_SOC] > 0 and t2[T_SOC] > 0
        for k in range(5):
            assert _close(terms[t, k], want[k]), (t, WEIGHT_NAMES[k], terms[t, k], want[k])
        assert np.all(np.abs(pts[t, KNOT + 1:] - opts[1:]) <= RTOL_F64 * np.maximum(np.abs(opts[1:]), 1.0)), t
    assert counted >= 2, (key, counted)
    g.close()
    g1.close()


# ---- 8. early ends ---------------------------------------------------------------------------------------------------------------------
def _lethal_scene():
    """a lethal block on the x axis 0.3 m ahead, point footprint, the one person far away (tests/test_crowd_gpu.py)"""
    base = syn.make_scene(_workload(1, 11, 0, footprint="point"))
    cells = base.cells.copy()
    my, mx = int((0.0 - base.origin_y) / base.resolution), int((0.3 - base.origin_x) / base.resolution)
    cells[my - 1:my + 1, mx:mx + 2] = 254
    agents = _copy_agents(base)
    p = agents[1]
    p.x, p.y, p.vx, p.vy, p.goal_x, p.goal_y = -3.0, -3.0, -0.5, -0.5, -4.0, -4.0
    return dataclasses.replace(base, cells=cells, agents=agents)


def _contact_scene():
    """one slow person standing 0.7 m ahead on the robot's axis"""
    base = _scene((1, 11, 0))
    agents = _copy_agents(base)
    p = agents[1]
    p.x, p.y, p.vx, p.vy, p.has_goal, p.desired_velocity = 0.7, 0.0, 0.0, 0.0, 0, 0.05
    return dataclasses.replace(base, agents=agents)


EARLY_C1, EARLY_C2 = (0.5, 0.0), (0.7, 0.0)  # 0.17 m in the first 12 steps; the block / the person are reached behind the knot


@pytest.mark.parametrize("precision", PRECISIONS)
def test_illegal_footprint_in_the_second_segment(oracle_mod, hip_mod, precision):
    scene = _lethal_scene()
    ok1, _, _ = _oracle_terms(oracle_mod, scene, None, scene.robot_state, EARLY_C1, 0.375)
    assert ok1  # only the second segment reaches the block
    g, g1 = _scorer(hip_mod, scene, precision), _scorer(hip_mod, scene, precision)
    rs_k, agents_k = _continuation(g1, scene, EARLY_C1)
    o = _oracle(oracle_mod, scene, agents=agents_k, sim_time=0.625)
    oc, opts = o.score_one(rs_k, EARLY_C2[0], 0.0, EARLY_C2[1], scene.goal_args)
    o.close()
    j = len(opts)
    assert oc == -1.0 and 0 < j < S - KNOT
    vx, vth = _two_knots([(EARLY_C1, EARLY_C2), (EARLY_C1, EARLY_C1)])
    g.set_terms_capture(True)
    costs, best = g.score_sequences(scene.robot_state, vx, vth, (0, KNOT), scene.goal_args)
    assert costs[0] == SFW_COST_INVALID and np.all(g.cost_terms()[0] == SFW_COST_INVALID)
    pts, npts = g.grid_points_batch(0, 2, S)
    assert npts[0] == KNOT + j, (npts, j)
    assert np.all(np.abs(pts[0, KNOT:KNOT + j] - opts) <= RTOL_F64 * np.maximum(np.abs(opts), 1.0))
    d = g.grid_crowd(0)
    assert d["cost"] == SFW_COST_INVALID and d["n_steps"] == KNOT + j
    assert best["n_valid"] == int(np.sum(costs >= 0))
    g.close()
    g1.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_pedestrian_contact_in_the_second_segment(oracle_mod, hip_mod, precision):
    scene = _contact_scene()
    ok1, _, _ = _oracle_terms(oracle_mod, scene, None, scene.robot_state, EARLY_C1, 0.375)
    assert ok1  # only the second segment touches the person
    g, g1 = _scorer(hip_mod, scene, precision), _scorer(hip_mod, scene, precision)
    rs_k, agents_k = _continuation(g1, scene, EARLY_C1)
    o = _oracle(oracle_mod, scene, agents=agents_k, sim_time=0.625)
    oc, opts = o.score_one(rs_k, EARLY_C2[0], 0.0, EARLY_C2[1], scene.goal_args)
    o.close()
    c = len(opts) - 1  # the continuation's contact step
    assert oc == -1.0 and 0 < c < S - KNOT - 1
    vx, vth = _two_knots([(EARLY_C1, EARLY_C2)])
    g.set_terms_capture(True)
    costs, best = g.score_sequences(scene.robot_state, vx, vth, (0, KNOT), scene.goal_args)
    assert costs[0] == SFW_COST_INVALID and np.all(g.cost_terms()[0] == SFW_COST_INVALID)
    assert best["index"] == -1 and best["n_valid"] == 0
    d = g.grid_crowd(0)
    assert d["cost"] == SFW_COST_INVALID and d["n_steps"] == KNOT + c + 1, (d["n_steps"], c)
    assert len(g.grid_points(0)) == KNOT + c + 1
    rr = float(np.float32(0.35) * np.float32(0.35))  # float-squared, ref :617
    dx, dy = d["state"][:, 0, 0] - d["state"][:, 1, 0], d["state"][:, 0, 1] - d["state"][:, 1, 1]
    touch = dx * dx + dy * dy <= rr
    assert touch[KNOT + c] and not np.any(touch[:KNOT + c])
    g.close()
    g1.close()


# ---- 9. state and arguments -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_staged_list_alone(hip_mod):
    scene = _scene((5, 12, 0))
    lx, ly, lth = _commands(20, 37)
    vx, vy, vth = _commands(6, 38, K=3)
    g = _scorer(hip_mod, scene)
    costs, best = g.score_samples(scene.robot_state, lx[0], lth[0], HOLO_GA, vy=ly[0])
    g.stage_samples(scene.robot_state, lx[0], lth[0], HOLO_GA, vy=ly[0])
    L = hip_mod.lib()
    rs, ga = hip_mod.SfwRobotState(*scene.robot_state), hip_mod.SfwGoalArgs(*HOLO_GA)
    ks = np.array([0, 7, 19], dtype=np.int32)
    many = np.arange(65, dtype=np.int32)
    wide = np.zeros((65, 6))

    def call(rs_p=C.byref(rs), vx_p=vx.ctypes.data, vy_p=vy.ctypes.data, vth_p=vth.ctypes.data, n=6, K=3, ks_p=ks.ctypes.data,
             ga_p=C.byref(ga)):
        return L.sfw_sequences_stage(g._h, rs_p, vx_p, vy_p, vth_p, n, K, ks_p, ga_p, 0)

    def knots(*v):
        return np.array(v, dtype=np.int32)

    def with_bad(a, value, at=(1, 3)):
        b = a.copy()
        b[at] = value
        return b

    bad_rs = hip_mod.SfwRobotState(0.0, np.nan, 0.0, 0.3, 0.0, 0.0)
    bad_ga = hip_mod.SfwGoalArgs(1.0, 0.7, np.inf, 2.0, 0.5)
    k_first, k_equal, k_down = knots(1, 7, 19), knots(0, 7, 7), knots(0, 19, 7)
    b_vx, b_vy, b_vth = with_bad(vx, np.nan), with_bad(vy, np.inf, (2, 0)), with_bad(vth, -np.inf, (0, 5))
    refused = [call(n=0), call(n=-3), call(K=0), call(K=-1), call(K=65, vx_p=wide.ctypes.data, vy_p=None, vth_p=wide.ctypes.data,
                                                                    ks_p=many.ctypes.data),
               call(rs_p=None), call(vx_p=None), call(vth_p=None), call(ks_p=None), call(ga_p=None),
               call(ks_p=k_first.ctypes.data), call(ks_p=k_equal.ctypes.data), call(ks_p=k_down.ctypes.data),
               call(vx_p=b_vx.ctypes.data), call(vy_p=b_vy.ctypes.data), call(vth_p=b_vth.ctypes.data),
               call(rs_p=C.byref(bad_rs)), call(ga_p=C.byref(bad_ga)),
               L.sfw_sequences_stage(None, C.byref(rs), vx.ctypes.data, None, vth.ctypes.data, 6, 3, ks.ctypes.data, C.byref(ga), 0)]
    assert refused == [SFW_ERR_INVALID_ARG] * len(refused), refused
    g.launch()  # the list is still staged
    c2, b2, _ = g.fetch()
    assert _same(c2, costs) and b2 == best
    assert call(K=64, vx_p=wide.ctypes.data, vy_p=None, vth_p=wide.ctypes.data, ks_p=many.ctypes.data) == 0  # SFW_SEQ_MAX_KNOTS
    assert call(vy_p=None) == 0
    g.close()
    # no costmap
    e = hip_mod.HipScorer(_params())
    with pytest.raises(hip_mod.SfwError) as err:
        e.stage_sequences((0, 0, 0, 0, 0, 0), [[0.1], [0.2]], [[0.0], [0.1]], [0, 5], HOLO_GA)
    assert err.value.status == SFW_ERR_STATE
    e.close()


def test_grid_list_and_sequences_replace_one_another(hip_mod):
    scene = _scene((5, 12, 0))
    lin, ang = syn.reference_sampler()
    lx, ly, lth = _commands(20, 37)
    vx, vy, vth = _commands(30, 38, K=3)
    steps = (0, 7, 19)
    rs = scene.robot_state
    g = _scorer(hip_mod, scene)
    gc, gb = g.score_grid(rs, lin, ang, scene.goal_args)
    lc, lb = g.score_samples(rs, lx[0], lth[0], HOLO_GA, vy=ly[0])
    sc, sb = g.score_sequences(rs, vx, vth, steps, HOLO_GA, vy=vy)
    stage = {"grid": lambda: g.stage(rs, lin, ang, scene.goal_args), "list": lambda: g.stage_samples(rs, lx[0], lth[0], HOLO_GA, vy=ly[0]),
             "seq": lambda: g.stage_sequences(rs, vx, vth, steps, HOLO_GA, vy=vy)}
    want = {"grid": (gc, gb, 45), "list": (lc, lb, 20), "seq": (sc, sb, 30)}
    for first, then in (("grid", "seq"), ("seq", "grid"), ("list", "seq"), ("seq", "list"), ("seq", "seq")):
        stage[first]()
        stage[then]()
        assert g.plan_info()["samples"] == want[then][2]
        g.launch()
        c, b, _ = g.fetch()
        assert _same(c, want[then][0]) and b == want[then][1], (first, then)
    # the scalar call consumes staged sequences
    stage["seq"]()
    g.score_one(rs, 0.3, 0.0, 0.1, scene.goal_args)
    with pytest.raises(hip_mod.SfwError) as e:
        g.launch()
    assert e.value.status == SFW_ERR_STATE
    # a new step count between stage and launch: the knots are looked up as the steps go by
    stage["seq"]()
    g.set_params(_params(sim_time=0.5))  # 16 steps: the knot at 19 is past the horizon now
    g.launch()
    c16, b16, _ = g.fetch()
    f = hip_mod.HipScorer(_params(sim_time=0.5))
    f.load_scene(scene)
    f16, fb16 = f.score_sequences(rs, vx[:2], vth[:2], steps[:2], HOLO_GA, vy=vy[:2])
    assert _same(c16, f16) and b16 == fb16
    f.close()
    g.close()


def test_batch_with_a_sequence_a_list_and_a_grid_member(hip_mod):
    scene = _scene((5, 12, 0))
    lin, ang = syn.reference_sampler()
    lx, ly, lth = _commands(20, 37)
    vx, vy, vth = _commands(30, 38, K=3)
    steps = (0, 7, 19)
    rs, ga = scene.robot_state, scene.goal_args
    alone = _scorer(hip_mod, scene)
    want = [alone.score_sequences(rs, vx, vth, steps, HOLO_GA, vy=vy), alone.score_samples(rs, lx[0], lth[0], HOLO_GA, vy=ly[0]),
            alone.score_grid(rs, lin, ang, ga)]
    alone.close()
    bs = hip_mod.BatchScorer(_params(), B=3)
    for i in range(3):
        bs.member(i).load_scene(scene)
    bs.member(0).stage_sequences(rs, vx, vth, steps, HOLO_GA, vy=vy)
    bs.member(1).stage_samples(rs, lx[0], lth[0], HOLO_GA, vy=ly[0])
    bs.stage(2, rs, lin, ang, ga)
    bs.launch()
    bests = bs.fetch()
    for i in range(3):
        costs = bs.member(i).costs_view().copy()
        assert _same(costs, want[i][0]), (i, np.flatnonzero(_bits(costs) != _bits(want[i][0])))
        assert bests[i] == want[i][1], (i, bests[i], want[i][1])
    d = bs.describe()
    assert d["members"] == 3 and d["one_launch_members"] == 1 and d["own_path_members"] == 2, d
    bs.close()


# ---- 10. a pinned person ---------------------------------------------------------------------------------------------------------------
def _pinned_scene(robot_vx):
    """(5, 12, 0) with person 1 pinned (desired_velocity 0, standing 1.2 m ahead to the left) and the robot handed over at
    robot_vx"""
    base = _scene((5, 12, 0))
    agents = _copy_agents(base)
    p = agents[1]
    p.x, p.y, p.vx, p.vy, p.has_goal, p.desired_velocity = 1.2, 0.4, 0.0, 0.0, 0, 0.0
    agents[0].vx = robot_vx
    rs = (0.0, 0.0, 0.0, robot_vx, 0.0, 0.0)
    return dataclasses.replace(base, agents=agents, robot_state=rs)


@pytest.mark.parametrize("precision", F64_MODES)
def test_pinned_person_robot_stands_until_a_knot(oracle_mod, hip_mod, precision):
    """Case A: the robot stands at hand-over, the sequence is (0, 0, 0) until step 12, then c2.  It is at rest at the
    handed-over pose only, which the pinned-rest table covers step by step: the flag stays 0 and the social term is the
    oracle's W12(standing) + W'(c2 from the world after 12 standing steps) within RTOL_F64."""
    scene = _pinned_scene(0.0)
    stand, c2 = (0.0, 0.0), (0.5, 0.2)
    g, g1 = _scorer(hip_mod, scene, precision, **SOCIAL_ONLY), _scorer(hip_mod, scene, precision, **SOCIAL_ONLY)
    vx, vth = _two_knots([(stand, c2)])
    g.stage_sequences(scene.robot_state, vx, vth, (0, KNOT), scene.goal_args)
    assert g.plan_info()["rest_noise_unreproduced"] == 0
    g.launch()
    costs, _, _ = g.fetch()
    rs_k, agents_k = _continuation(g1, scene, stand)
    o = _oracle(oracle_mod, scene, sim_time=0.375, **SOCIAL_ONLY)
    w1 = o.score_one(scene.robot_state, 0.0, 0.0, 0.0, scene.goal_args)[0]
    o.close()
    o = _oracle(oracle_mod, scene, agents=agents_k, sim_time=0.625, **SOCIAL_ONLY)
    w2 = o.score_one(rs_k, c2[0], 0.0, c2[1], scene.goal_args)[0]
    o.close()
    print(f"pinned, standing until {KNOT}: social {costs[0]!r}, oracle {w1!r} + {w2!r}, rel {abs(costs[0] - (w1 + w2)) / (w1 + w2):.3e}")
    assert w1 > 0 and w2 > 0
    assert abs(costs[0] - (w1 + w2)) <= RTOL_F64 * (w1 + w2)
    g.close()
    g1.close()


def test_pinned_person_robot_brakes_to_rest_behind_a_knot(hip_mod):
    """Case B: the robot moves at hand-over; c1 until step 12, then (0, 0, 0) under an acceleration limit of 2 m/s^2: 0.5 m/s
    are gone 8 steps later, before step 30 — the configuration the kernels do not reproduce, flagged."""
    scene = _pinned_scene(float(np.float32(0.3)))
    ga = (2.0, 0.0, 1.0, 2.0, 0.5)
    g = _scorer(hip_mod, scene)
    vx, vth = _two_knots([((0.5, 0.2), (0.0, 0.0)), ((0.5, 0.2), (0.5, 0.2))])
    g.stage_sequences(scene.robot_state, vx, vth, (0, KNOT), ga)
    assert g.plan_info()["rest_noise_unreproduced"] == 1
    # the same commands never coming to rest: no flag; nobody pinned: no flag
    g.stage_sequences(scene.robot_state, vx[:, 1:], vth[:, 1:], (0, KNOT), ga)
    assert g.plan_info()["rest_noise_unreproduced"] == 0
    free = _scorer(hip_mod, _scene((5, 12, 0)))
    free.stage_sequences(scene.robot_state, vx, vth, (0, KNOT), ga)
    assert free.plan_info()["rest_noise_unreproduced"] == 0
    free.close()
    g.close()
