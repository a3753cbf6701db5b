"""MPPI on the device (sfw_sequences_control_cost, sfw_grid_blend_control, sfw_mppi_run), held to include/sfw_hip.h:
  1. control cost: the device's vector is bitwise mppi.control_cost fed the device's own normals, with and without
     SFW_PERTURB_KEEP_NORMALS, before and after the launch, at an index_base whose counter carries;
  2. blend with the control cost: bitwise sfw_grid_blend with that vector as its bias; gamma == 0 is the plain blend;
  3. chain: sfw_mppi_run equals the loop of calls it is defined by, run on a second handle, in everything it produces;
  4. no valid rollout; 5. refusals and state.
"Bitwise" compares uint64 views.  The scenes are the synthetic 32-step scenes of tests/test_perturb_gpu.py."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from social_force_window_planner_amd import mppi
from social_force_window_planner_amd import synthetic as syn
from social_force_window_planner_amd._abi import (SFW_COST_INVALID, SFW_ERR_INVALID_ARG, SFW_ERR_STATE, SFW_PERTURB_KEEP_NOMINAL,
                                                   SFW_PERTURB_KEEP_NORMALS, SFW_PERTURB_NO_VY, SfwBest, SfwBlendStat, SfwMppi,
                                                   SfwPerturb)
from sfw_test_util import _bits, _knot_steps, _nominal, _params, _same, _scorer, _workload

pytestmark = pytest.mark.gpu

GRAN = 0.03125
STEPS = 32
HOLO_GA = (1.0, 0.7, 1.0, 2.0, 0.5)
L16 = [float(x) for x in np.geomspace(1e-3, 1e3, 16)]
KEEP, NO_VY, NOMINAL = SFW_PERTURB_KEEP_NORMALS, SFW_PERTURB_NO_VY, SFW_PERTURB_KEEP_NOMINAL
SIGMA = (0.2, 0.1, 0.3)
WIDE = ((0.0, -0.3, -0.5), (0.7, 0.3, 0.5))  # the robot's limits


# ---- the scenes and helpers of tests/test_perturb_gpu.py ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(key):
    """(cached and never written to)"""
    if key == "lethal":  # a lethal block on the x axis 0.3 m ahead, point footprint
        base = syn.make_scene(_workload(5, 12, 0, footprint="point"))
        cells = base.cells.copy()
        my, mx = int((0.0 - base.origin_y) / base.resolution), int((0.3 - base.origin_x) / base.resolution)
        cells[my - 1:my + 1, mx:mx + 2] = 254
        return dataclasses.replace(base, cells=cells)
    if key == "walled":  # lethal everywhere: no rollout is valid
        base = syn.make_scene(_workload(5, 12, 0))
        return dataclasses.replace(base, cells=np.full_like(base.cells, 254))
    if key == "pinned":  # (5, 12, 0) with person 1 pinned: desired_velocity 0, standing 1.2 m ahead to the left
        base = syn.make_scene(_workload(5, 12, 0))
        agents = (type(base.agents[0]) * len(base.agents))()
        for a in range(len(base.agents)):
            C.memmove(C.byref(agents[a]), C.byref(base.agents[a]), C.sizeof(agents[a]))
        p = agents[1]
        p.x, p.y, p.vx, p.vy, p.has_goal, p.desired_velocity = 1.2, 0.4, 0.0, 0.0, 0, 0.0
        return dataclasses.replace(base, agents=agents)
    return syn.make_scene(_workload(*key))


def _stat_bits(stats):
    return [sorted((k, _bits(float(v)).item()) for k, v in d.items()) for d in stats]


def _stage(g, scene, n, K, seed, flags=0, sigma=SIGMA, index_base=0):
    no_vy = bool(flags & NO_VY)
    nominal = _nominal(K, no_vy)
    sigma = (sigma[0], 0.0, sigma[2]) if no_vy else sigma
    g.stage_perturbed(scene.robot_state, n, seed, nominal, sigma, WIDE[0], WIDE[1], _knot_steps(K), HOLO_GA, flags=flags,
                      index_base=index_base)
    return nominal, sigma


# ---- 1. the control cost ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 515])
def test_control_cost_is_the_mirror_of_the_device_normals(hip_mod, n):
    scene = _scene((5, 12, 0))
    g = _scorer(hip_mod, scene)
    for K in (1, 3, 64):
        for flags in (0, NO_VY, NOMINAL):
            for sigma in (SIGMA, (0.2, 0.1, 0.0)):  # ... and a channel that is not perturbed
                seed, gamma = 1000 * n + 10 * K + flags, 0.3 + 0.01 * K
                nominal, sig = _stage(g, scene, n, K, seed, flags | KEEP, sigma)
                z = g.normals(0, n)
                want = mppi.control_cost(nominal, sig, z, gamma)
                kept_before = g.control_cost(gamma)
                g.launch()
                g.fetch()
                kept_after = g.control_cost(gamma)
                _stage(g, scene, n, K, seed, flags, sigma)  # the normals are not kept: they are drawn again
                drawn_before = g.control_cost(gamma)
                g.launch()
                costs, best, _ = g.fetch()
                drawn_after = g.control_cost(gamma)
                for name, got in (("kept", kept_before), ("kept, launched", kept_after), ("drawn", drawn_before),
                                  ("drawn, launched", drawn_after)):
                    assert got.shape == (n,) and _same(got, want), (K, flags, sigma, name, np.flatnonzero(_bits(got) != _bits(want))[:4])
                if flags & NOMINAL:
                    assert want[0] == 0.0 and kept_before[0] == 0.0  # (+0.0 or -0.0: z == 0 in every term)
                assert n < 63 or len(np.unique(want)) > n // 2
                zero = g.control_cost(0.0)
                assert np.all(zero == 0.0)
                # read-only for the launch
                c2, b2, _ = g.fetch()
                assert _same(c2, costs) and b2 == best
    g.close()


def test_control_cost_where_the_counter_carries(hip_mod):
    scene = _scene((20, 14, 16))
    g = _scorer(hip_mod, scene)
    base, n, K, seed = 2 ** 32 - 3, 8, 3, (0x9E3779B9 << 32) | 0x7F4A7C15
    nominal, sigma = _stage(g, scene, n, K, seed, KEEP | NOMINAL, index_base=base)
    want = mppi.control_cost(nominal, sigma, g.normals(0, n), -1.25)
    assert _same(g.control_cost(-1.25), want) and not np.any(want == 0.0)  # (global sample 0 is not in this shard)
    _stage(g, scene, n, K, seed, NOMINAL, index_base=base)
    assert _same(g.control_cost(-1.25), want)
    # the shard's values are the unsharded stage's: (seed, g) alone
    _stage(g, scene, 5, K, seed, 0, index_base=base + 3)
    assert _same(g.control_cost(-1.25), want[3:])
    g.close()


# ---- 2. the blend with the control cost ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K,flags", [(257, 3, 0), (515, 4, NO_VY | KEEP), (64, 1, NOMINAL)])
def test_blend_control_is_the_blend_with_the_control_cost_as_bias(hip_mod, n, K, flags):
    scene = _scene("lethal")
    g = _scorer(hip_mod, scene)
    _stage(g, scene, n, K, 900 + n, flags)
    g.launch()
    costs, best, _ = g.fetch()
    assert 0 < best["n_valid"] < n
    gamma = 0.3
    cc = g.control_cost(gamma)
    extra = np.random.default_rng(n).normal(0.0, 0.2, n)
    for lam in ([0.7], L16):
        got = g.blend(lam, gamma=gamma, want_weights=True)
        want = g.blend(lam, bias=cc, want_weights=True)
        assert _stat_bits(got[0]) == _stat_bits(want[0]) and _same(got[1], want[1]) and _same(got[2], want[2])
        got = g.blend(lam, gamma=gamma, bias=extra, want_weights=True)
        want = g.blend(lam, bias=cc + extra, want_weights=True)
        assert _stat_bits(got[0]) == _stat_bits(want[0]) and _same(got[1], want[1]) and _same(got[2], want[2])
        plain = g.blend(lam, want_weights=True)
        zero = g.blend(lam, gamma=0.0, want_weights=True)
        assert _stat_bits(zero[0]) == _stat_bits(plain[0]) and _same(zero[1], plain[1]) and _same(zero[2], plain[2])
        plain_b = g.blend(lam, bias=extra, want_weights=True)
        zero_b = g.blend(lam, gamma=0.0, bias=extra, want_weights=True)
        assert _stat_bits(zero_b[0]) == _stat_bits(plain_b[0]) and _same(zero_b[1], plain_b[1]) and _same(zero_b[2], plain_b[2])
        # gamma matters
        got = g.blend(lam, gamma=gamma)
        assert _stat_bits(got[0]) != _stat_bits(plain[0]) and not _same(got[1], plain[1])
    c2, b2, _ = g.fetch()  # read-only for the launch
    assert _same(c2, costs) and b2 == best
    g.close()


# ---- 3. the chain ----------------------------------------------------------------------------------------------------------------------
def _loop(g, scene, n, K, seed, nominal, sigma, iterations, lam, gamma, flags):
    """sfw_mppi_run's definition, call by call"""
    nom, stats, plans, best = np.array(nominal, dtype=np.float64), [], [], None
    for i in range(iterations):
        g.stage_perturbed(scene.robot_state, n, (seed + i) % 2 ** 64, nom, sigma, WIDE[0], WIDE[1], _knot_steps(K), HOLO_GA, flags=flags)
        g.launch()
        _, best, _ = g.fetch(want_costs=False)
        st, u, _ = g.blend([lam], gamma=gamma)
        if st[0]["n_valid"] > 0:
            nom = u[0].copy()
        stats.append(st[0])
        plans.append(nom.copy())
    return stats, np.stack(plans), best


def _everything(g, n, K, best):
    costs, b, key = g.fetch()
    out = {"costs": costs.copy(), "best": b, "key": key, "knots": g.knots(0, n), "terms": g.cost_terms()}
    if best["index"] >= 0:
        out["points"] = g.grid_points(best["index"])
        crowd = g.grid_crowd(best["index"])
        out["crowd"] = [crowd[f] for f in ("state", "work", "cost")]
    return out


def _hold_chain(a, b, scene, n, K, seed, iterations, gamma, flags, lam=0.05):
    no_vy = bool(flags & NO_VY)
    nominal, sigma = _nominal(K, no_vy), (SIGMA[0], 0.0, SIGMA[2]) if no_vy else SIGMA
    stats, plans, best = a.mppi_run(scene.robot_state, n, seed, nominal, sigma, WIDE[0], WIDE[1], _knot_steps(K), HOLO_GA, iterations, lam,
                                    gamma, flags=flags)
    w_stats, w_plans, w_best = _loop(b, scene, n, K, seed, nominal, sigma, iterations, lam, gamma, flags)
    case = (n, K, iterations, gamma, flags)
    assert plans.shape == (iterations, K, 3) and np.all(np.isfinite(plans))
    assert _stat_bits(stats) == _stat_bits(w_stats), case
    assert _same(plans, w_plans), case
    assert best == w_best and all(_same(best[f], w_best[f]) for f in ("cost", "vx", "vy", "vtheta")), case
    got, want = _everything(a, n, K, best), _everything(b, n, K, w_best)
    assert got["best"] == best and got["key"] == want["key"]
    for f in ("costs", "knots", "terms", "points"):
        if f in want:
            assert _same(got[f], want[f]), (case, f)
    for x, y in zip(got.get("crowd", []), want.get("crowd", [])):
        assert _same(x, y), case
    # the stage the handle holds is the last iteration's: the control cost and the blend act on it
    assert _same(a.control_cost(0.7), b.control_cost(0.7)), case
    ga_, gb_ = a.blend(L16, gamma=0.7), b.blend(L16, gamma=0.7)
    assert _stat_bits(ga_[0]) == _stat_bits(gb_[0]) and _same(ga_[1], gb_[1]), case
    if flags & KEEP:
        assert _same(a.normals(0, n), b.normals(0, n)), case
    if flags & NOMINAL:  # sample 0 of the last iteration is the plan it was drawn around
        before = plans[iterations - 2] if iterations > 1 else nominal
        assert _same(got["knots"][:, :, 0], before), case
    if n >= 64:
        assert 0 < stats[-1]["n_valid"] < n, (case, [s["n_valid"] for s in stats])
        assert np.any(got["costs"] == SFW_COST_INVALID) and np.any(got["costs"] >= 0)
        steps = np.concatenate([nominal[None], plans])
        for i in range(iterations):
            assert np.any(_bits(steps[i]) != _bits(steps[i + 1])), (case, i)
    return stats, plans, best


@pytest.mark.parametrize("n", [1, 64, 257, 515])
def test_mppi_run_is_the_loop_it_is_defined_by(hip_mod, n):
    scene = _scene("lethal")
    a, b = _scorer(hip_mod, scene), _scorer(hip_mod, scene)
    for h in (a, b):
        h.set_terms_capture(True)
    for K, flags in ((1, 0), (4, NOMINAL | KEEP), (4, NO_VY)):
        for iterations in (1, 2, 5):
            for gamma in (0.0, 0.3):
                if (K, flags) == (4, NO_VY) and (iterations != 2 or gamma == 0.0):
                    continue
                _hold_chain(a, b, scene, n, K, 7000 + 10 * n + iterations, iterations, gamma, flags)
    a.close()
    b.close()


def test_mppi_run_on_every_scoring_path(hip_mod, monkeypatch):
    scene = _scene("lethal")
    ref = _scorer(hip_mod, scene)
    ref.set_terms_capture(True)

    def fresh():
        h = _scorer(hip_mod, scene)
        h.set_terms_capture(True)
        return h

    plain = fresh()
    _hold_chain(plain, ref, scene, 64, 4, 31, 2, 0.3, NOMINAL)
    assert plain.plan_info()["one_launch"] == 1
    monkeypatch.setenv("SFW_CYCLE_FUSED", "0")
    unfused = fresh()
    _hold_chain(unfused, ref, scene, 64, 4, 31, 2, 0.3, NOMINAL)
    assert unfused.plan_info()["one_launch"] == 0
    monkeypatch.delenv("SFW_CYCLE_FUSED")
    monkeypatch.setenv("SFW_TABLE_BUDGET_MB", "1")
    chunked = fresh()
    monkeypatch.delenv("SFW_TABLE_BUDGET_MB")
    _hold_chain(chunked, ref, scene, 2100, 4, 32, 2, 0.3, 0)
    assert chunked.plan_info()["chunks"] > 1
    monkeypatch.setenv("SFW_DEVICE_CUS", "32")
    small = fresh()
    monkeypatch.delenv("SFW_DEVICE_CUS")
    _hold_chain(small, ref, scene, 2100, 4, 32, 2, 0.3, 0)
    _hold_chain(small, ref, scene, 515, 1, 33, 5, 0.3, KEEP)
    for h in (ref, plain, unfused, chunked, small):
        h.close()


def test_other_scenes_and_seeds_near_the_top(hip_mod):
    a, b = _scorer(hip_mod, _scene((20, 14, 16))), _scorer(hip_mod, _scene((20, 14, 16)))
    for h in (a, b):
        h.set_terms_capture(True)
    scene = _scene((20, 14, 16))
    nominal = _nominal(3)
    for seed in (2 ** 64 - 2, 5):  # seed + i wraps modulo 2^64
        got = a.mppi_run(scene.robot_state, 130, seed, nominal, SIGMA, WIDE[0], WIDE[1], _knot_steps(3), HOLO_GA, 4, 0.05, 0.3)
        want = _loop(b, scene, 130, 3, seed, nominal, SIGMA, 4, 0.05, 0.3, 0)
        assert _stat_bits(got[0]) == _stat_bits(want[0]) and _same(got[1], want[1]) and got[2] == want[2]
        assert _same(a.fetch()[0], b.fetch()[0]) and _same(a.knots(0, 130), b.knots(0, 130))
    p, q = _scorer(hip_mod, _scene("pinned")), _scorer(hip_mod, _scene("pinned"))
    scene = _scene("pinned")
    got = p.mppi_run(scene.robot_state, 257, 9, nominal, SIGMA, WIDE[0], WIDE[1], _knot_steps(3), HOLO_GA, 3, 0.05, 0.3)
    want = _loop(q, scene, 257, 3, 9, nominal, SIGMA, 3, 0.05, 0.3, 0)
    assert _stat_bits(got[0]) == _stat_bits(want[0]) and _same(got[1], want[1]) and got[2] == want[2]
    assert p.plan_info() == q.plan_info()
    for h in (a, b, p, q):
        h.close()


# ---- 4. no valid rollout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257])
def test_no_valid_rollout_keeps_the_nominal(hip_mod, n):
    scene = _scene("walled")
    g = _scorer(hip_mod, scene)
    nominal = _nominal(4)
    for gamma in (0.0, 0.3):
        stats, plans, best = g.mppi_run(scene.robot_state, n, 3, nominal, SIGMA, WIDE[0], WIDE[1], _knot_steps(4), HOLO_GA, 3, 0.5, gamma)
        for s in stats:
            assert (s["lambda"], s["j_min"], s["eta"], s["sum_w2"], s["n_valid"], s["index_min"]) == (0.5, -1.0, 0.0, 0.0, 0, -1)
            assert _bits(s["eta"]).item() == 0 and _bits(s["sum_w2"]).item() == 0
        for i in range(3):
            assert _same(plans[i], nominal)
        assert best["index"] == -1 and best["n_valid"] == 0
        assert np.all(g.fetch()[0] == SFW_COST_INVALID)
    g.close()


# ---- 5. refusals and state -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_staged_grid_alone(hip_mod):
    scene = _scene((5, 12, 0))
    g = _scorer(hip_mod, scene)
    lin, ang = syn.reference_sampler()
    costs, best = g.score_grid(scene.robot_state, lin, ang, scene.goal_args)
    L = hip_mod.lib()
    rs, ga = hip_mod.SfwRobotState(*scene.robot_state), hip_mod.SfwGoalArgs(*HOLO_GA)
    ks = np.array([0, 7, 19], dtype=np.int32)
    nom = np.ascontiguousarray(_nominal(3))
    keep = []

    def perturb_of(nominal=nom, sigma=SIGMA, lo=WIDE[0], hi=WIDE[1], flags=0, reserved=0, null_nominal=False):
        p = SfwPerturb()
        p.seed = 1
        a = np.ascontiguousarray(nominal, dtype=np.float64)
        keep.append(a)
        p.nominal = None if null_nominal else a.ctypes.data
        p.sigma, p.lo, p.hi = (C.c_double * 3)(*sigma), (C.c_double * 3)(*lo), (C.c_double * 3)(*hi)
        p.flags, p.reserved = flags, reserved
        return p

    stat, plans, sel = (SfwBlendStat * 32)(), np.zeros((32, 3, 3)), SfwBest()

    def run(p=None, m=(2, 0, 0.5, 0.3), rs_p=C.byref(rs), n=6, K=3, ks_p=ks.ctypes.data, ga_p=C.byref(ga), null_p=False, null_m=False,
            stat_p=stat, plans_p=plans.ctypes.data, h=g._h):
        p = perturb_of() if p is None else p
        mm = SfwMppi(*m)
        return L.sfw_mppi_run(h, rs_p, None if null_p else C.byref(p), n, K, ks_p, ga_p, None if null_m else C.byref(mm), stat_p,
                              plans_p, C.byref(sel))

    def knots(*v):
        a = np.array(v, dtype=np.int32)
        keep.append(a)
        return a.ctypes.data

    bad_nom = nom.copy()
    bad_nom[1, 0] = np.nan
    lam = np.array([0.5])
    u = np.zeros((16, 64, 3))
    out = np.zeros(64)

    def checked():
        refused = [
            run(h=None), run(null_m=True), run(stat_p=None), run(plans_p=None),
            run(m=(0, 0, 0.5, 0.3)), run(m=(-1, 0, 0.5, 0.3)), run(m=(33, 0, 0.5, 0.3)), run(m=(2, 1, 0.5, 0.3)),
            run(m=(2, 0, 0.0, 0.3)), run(m=(2, 0, -0.5, 0.3)), run(m=(2, 0, np.nan, 0.3)), run(m=(2, 0, np.inf, 0.3)),
            run(m=(2, 0, 0.5, np.nan)), run(m=(2, 0, 0.5, np.inf)), run(m=(2, 0, 0.5, -np.inf)),
            # ... and what the perturbed stage refuses
            run(rs_p=None), run(null_p=True), run(perturb_of(null_nominal=True)), run(ks_p=None), run(ga_p=None),
            run(n=0), run(K=0), run(K=65), run(ks_p=knots(1, 7, 19)), run(ks_p=knots(0, 7, 7)),
            run(perturb_of(nominal=bad_nom)), run(perturb_of(sigma=(0.1, -0.1, 0.1))), run(perturb_of(lo=(0.8, -0.3, -0.5))),
            run(perturb_of(flags=8)), run(perturb_of(reserved=1)), run(perturb_of(flags=NO_VY)),
            run(rs_p=C.byref(hip_mod.SfwRobotState(0.0, np.nan, 0.0, 0.3, 0.0, 0.0))),
            # the control cost and its blend
            L.sfw_sequences_control_cost(None, 0.5, out.ctypes.data), L.sfw_sequences_control_cost(g._h, 0.5, None),
            L.sfw_sequences_control_cost(g._h, np.nan, out.ctypes.data), L.sfw_sequences_control_cost(g._h, np.inf, out.ctypes.data),
            L.sfw_grid_blend_control(None, lam.ctypes.data, 1, 0.5, None, stat, u.ctypes.data, None),
            L.sfw_grid_blend_control(g._h, None, 1, 0.5, None, stat, u.ctypes.data, None),
            L.sfw_grid_blend_control(g._h, lam.ctypes.data, 0, 0.5, None, stat, u.ctypes.data, None),
            L.sfw_grid_blend_control(g._h, lam.ctypes.data, 17, 0.5, None, stat, u.ctypes.data, None),
            L.sfw_grid_blend_control(g._h, lam.ctypes.data, 1, np.nan, None, stat, u.ctypes.data, None),
            L.sfw_grid_blend_control(g._h, lam.ctypes.data, 1, -np.inf, None, stat, u.ctypes.data, None),
            L.sfw_grid_blend_control(g._h, lam.ctypes.data, 1, 0.5, None, None, u.ctypes.data, None),
            L.sfw_grid_blend_control(g._h, lam.ctypes.data, 1, 0.5, None, stat, None, None),
            L.sfw_grid_blend_control(g._h, np.array([-1.0]).ctypes.data, 1, 0.5, None, stat, u.ctypes.data, None),
        ]
        assert refused == [SFW_ERR_INVALID_ARG] * len(refused), refused

    g.stage(scene.robot_state, lin, ang, scene.goal_args)
    checked()
    assert not np.any(plans) and stat[0].n_valid == 0  # a refused call writes nothing
    # a grid is staged: the control cost has nothing to act on
    assert L.sfw_sequences_control_cost(g._h, 0.5, out.ctypes.data) == SFW_ERR_STATE
    assert L.sfw_grid_blend_control(g._h, lam.ctypes.data, 1, 0.5, None, stat, u.ctypes.data, None) == SFW_ERR_STATE
    g.launch()  # the grid is still staged
    c2, b2, _ = g.fetch()
    assert _same(c2, costs) and b2 == best
    assert L.sfw_sequences_control_cost(g._h, 0.5, out.ctypes.data) == SFW_ERR_STATE
    assert L.sfw_grid_blend_control(g._h, lam.ctypes.data, 1, 0.5, None, stat, u.ctypes.data, None) == SFW_ERR_STATE
    # a non-finite bias is refused once there is something to size it by, and changes nothing
    _stage(g, scene, 6, 3, 1)
    assert L.sfw_grid_blend_control(g._h, lam.ctypes.data, 1, 0.5, None, stat, u.ctypes.data, None) == SFW_ERR_STATE  # not launched
    g.launch()
    pc, pb, _ = g.fetch()
    bad_bias = np.array([0.0, 0.0, np.inf, 0.0, 0.0, 0.0])
    assert L.sfw_grid_blend_control(g._h, lam.ctypes.data, 1, 0.5, bad_bias.ctypes.data, stat, u.ctypes.data, None) == SFW_ERR_INVALID_ARG
    checked()
    c3, b3, _ = g.fetch()
    assert _same(c3, pc) and b3 == pb
    # the limits themselves are accepted
    assert run(m=(32, 0, 1e-9, -1e6)) == 0 and run(m=(1, 0, 1e9, 0.0)) == 0
    g.close()
    # no costmap
    e = hip_mod.HipScorer(_params())
    with pytest.raises(hip_mod.SfwError) as err:
        e.mppi_run((0, 0, 0, 0, 0, 0), 4, 1, _nominal(2), SIGMA, WIDE[0], WIDE[1], (0, 5), HOLO_GA, 2, 0.5, 0.3)
    assert err.value.status == SFW_ERR_STATE
    with pytest.raises(hip_mod.SfwError) as err:  # nothing staged
        e.control_cost(0.5)
    assert err.value.status == SFW_ERR_STATE
    e.close()


def test_state_after_the_other_stages_and_after_the_run(hip_mod):
    scene = _scene("lethal")
    rs = scene.robot_state
    g = _scorer(hip_mod, scene)
    lx, lth = np.linspace(0.1, 0.6, 20), np.linspace(-0.4, 0.4, 20)
    vx, vth = np.tile(lx, (3, 1)), np.tile(lth, (3, 1)) * np.array([[1.0], [0.5], [-1.0]])
    for host_staged in (lambda: g.score_samples(rs, lx, lth, HOLO_GA), lambda: g.score_sequences(rs, vx, vth, (0, 7, 19), HOLO_GA)):
        host_staged()
        for call in (lambda: g.control_cost(0.5), lambda: g.blend([0.5], gamma=0.5)):
            with pytest.raises(hip_mod.SfwError) as e:
                call()
            assert e.value.status == SFW_ERR_STATE
        g.blend([0.5])  # (the plain blend serves them)
    nominal = _nominal(3)
    args = (rs, 130, 41, nominal, SIGMA, WIDE[0], WIDE[1], (0, 7, 19), HOLO_GA, 3, 0.05, 0.3)
    stats, plans, best = g.mppi_run(*args)
    costs = g.fetch()[0].copy()
    # the last iteration is a perturbed stage like any other: score_perturbed with its seed and nominal scores the same
    c2, b2 = g.score_perturbed(rs, 130, 43, plans[1], SIGMA, WIDE[0], WIDE[1], (0, 7, 19), HOLO_GA)
    assert _same(c2, costs) and b2 == best
    g.mppi_run(*args)
    g.launch()  # a re-launch
    c3, b3, _ = g.fetch()
    assert _same(c3, costs) and b3 == best
    # repeating the call gives the same bits
    s4, p4, b4 = g.mppi_run(*args)
    assert _stat_bits(s4) == _stat_bits(stats) and _same(p4, plans) and b4 == best
    # the scalar call consumes the stage
    g.score_one(rs, 0.3, 0.0, 0.1, scene.goal_args)
    for call in (g.launch, lambda: g.control_cost(0.5), lambda: g.blend([0.5], gamma=0.5), lambda: g.knots(0, 1)):
        with pytest.raises(hip_mod.SfwError) as e:
            call()
        assert e.value.status == SFW_ERR_STATE
    # another size, then the first again: the buffers grow and the bits stay
    g.mppi_run(rs, 2100, 41, _nominal(8), SIGMA, WIDE[0], WIDE[1], tuple(range(8)), HOLO_GA, 8, 0.05, 0.3)
    s5, p5, b5 = g.mppi_run(*args)
    assert _stat_bits(s5) == _stat_bits(stats) and _same(p5, plans) and b5 == best
    g.close()


def test_batch_member_runs_the_chain_on_its_own_path(hip_mod):
    scene = _scene("lethal")
    lin, ang = syn.reference_sampler()
    rs = scene.robot_state
    args = (rs, 130, 51, _nominal(3), SIGMA, WIDE[0], WIDE[1], (0, 7, 19), HOLO_GA, 3, 0.05, 0.3)
    alone = _scorer(hip_mod, scene)
    stats, plans, best = alone.mppi_run(*args)
    costs, cc = alone.fetch()[0].copy(), alone.control_cost(0.5)
    grid = alone.score_grid(rs, lin, ang, scene.goal_args)
    alone.close()
    bs = hip_mod.BatchScorer(_params(), B=2)
    for i in range(2):
        bs.member(i).load_scene(scene)
    m = bs.member(0)
    s2, p2, b2 = m.mppi_run(*args)
    assert _stat_bits(s2) == _stat_bits(stats) and _same(p2, plans) and b2 == best
    assert _same(m.fetch()[0], costs) and _same(m.control_cost(0.5), cc)
    # ... and the member's stage takes part in a batch launch as a perturbed stage does
    bs.stage(1, rs, lin, ang, scene.goal_args)
    bs.launch()
    bests = bs.fetch()
    assert bests[0] == best and bests[1] == grid[1] and _same(m.costs_view(), costs)
    assert bs.describe()["own_path_members"] == 1
    assert _same(m.control_cost(0.5), cc)
    bs.close()
