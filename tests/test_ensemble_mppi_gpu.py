"""sfw_ensemble_blend_control / sfw_ensemble_mppi_run: chained MPPI under several crowd hypotheses, held to include/sfw_hip.h:
  1. blend_control: the ensemble's blend with the control cost of a STANDALONE handle's stage of the same sfw_perturb as bias;
  2. M = 1: the chain is HipScorer.mppi_run on a standalone handle with the same scene;
  3. the chain equals the loop of single calls it is defined by, run on a second ensemble, in everything it produces and leaves;
  4. ... on scenes, sigma and lambda where that loop really updates the plan (asserted: a vacuous scene fails);
  5. no valid rollout; 6. refusals and state.
Everything is compared bitwise (uint64 views): no tolerance appears.  The mixed-hypothesis scene, its box, sigma and nominal
plan are those of tests/test_ensemble_sequences_gpu.py; the single-hypothesis scene is the "lethal" scene of
tests/test_mppi_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import golden_util as gu
import test_ensemble_sequences_gpu as es
import test_mppi_gpu as tm
from social_force_window_planner_amd._abi import (SFW_COST_INVALID, SFW_ERR_INVALID_ARG, SFW_ERR_STATE, SFW_OK, SFW_PERTURB_KEEP_NOMINAL,
                                                   SFW_PERTURB_KEEP_NORMALS, SFW_PERTURB_NO_VY, SfwBest, SfwBlendStat, SfwGoalArgs,
                                                   SfwMppi, SfwRobotState)

pytestmark = pytest.mark.gpu

KEEP, NO_VY, NOMINAL = SFW_PERTURB_KEEP_NORMALS, SFW_PERTURB_NO_VY, SFW_PERTURB_KEEP_NOMINAL
L16 = es.L16
_bits, _same = es._bits, es._same
_stat_bits = tm._stat_bits
SCENE = "ref5x9"
LAM = 1.0  # of the order of the cost differences between rollouts: the weights of many samples count (eta > 1)
PROBS3 = (0.5, 0.125, 0.375)


def _mixed3(scene):
    """M = 3 of the six mixed hypotheses: a naive-goal crowd, one with a person added, one with 60 laser points"""
    h = es._mixed_hypotheses(scene)
    return [h[0], h[4], h[5]]


def _case(n, K, flags, seed=None):
    """(seed, nominal, sigma, knot steps, goal args): a plan well inside the commands every hypothesis accepts, under a sigma
    that reaches the ones some and all of them reject.  n = 1 is a single rollout: a twentieth of that sigma keeps it, and the
    plans that follow it, among the accepted commands, so that every iteration of such a case updates the plan too"""
    no_vy = bool(flags & NO_VY)
    sigma = tuple(s / 20.0 for s in es.SIGMA) if n == 1 else es.SIGMA
    sigma = (sigma[0], 0.0, sigma[2]) if no_vy else sigma
    return (4100 + 10 * n + K if seed is None else seed, es._nominal(K, no_vy), sigma, es._perturbed_steps(K),
            es.NONH_GA if no_vy else es.HOLO_GA)


def _same_blend(a, b):
    return _stat_bits(a[0]) == _stat_bits(b[0]) and _same(a[1], b[1]) and (a[2] is None) == (b[2] is None) and \
        (a[2] is None or _same(a[2], b[2]))


# ---- 1. the blend with the control cost --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 515])
def test_blend_control_is_the_blend_with_the_control_cost_as_bias(hip_mod, n):
    scene = es._scene(SCENE)
    hyps = _mixed3(scene)
    g = es._standalone(hip_mod, scene, *hyps[0])
    rs = scene.robot_state
    gamma = 0.3
    extra = np.random.default_rng(n).normal(0.0, 0.2, n)
    differed = 0
    for M in (1, 3):
        e = es._ensemble(hip_mod, scene, hyps[:M])
        for K in (1, 3, 64):
            for flags in (0, NOMINAL, NO_VY, KEEP):
                seed, nominal, sigma, steps, ga = _case(n, K, flags)
                e.score_perturbed(rs, n, seed, nominal, sigma, es.WIDE[0], es.WIDE[1], steps, ga, flags=flags, mode="mean")
                # the term is a function of (seed, g, K, nominal, sigma, flags) alone: any handle that stages this sfw_perturb has it
                g.stage_perturbed(rs, n, seed, nominal, sigma, es.WIDE[0], es.WIDE[1], steps, ga, flags=flags)
                cc = g.control_cost(gamma)
                for lam in ([0.7], L16):
                    case = (M, K, flags, len(lam))
                    assert _same_blend(e.blend(lam, gamma=gamma, want_weights=True), e.blend(lam, bias=cc, want_weights=True)), case
                    assert _same_blend(e.blend(lam, gamma=gamma, bias=extra, want_weights=True),
                                       e.blend(lam, bias=cc + extra, want_weights=True)), case
                    plain = e.blend(lam, want_weights=True)
                    assert _same_blend(e.blend(lam, gamma=0.0, want_weights=True), plain), case
                    assert _same_blend(e.blend(lam, gamma=0.0, bias=extra, want_weights=True),
                                       e.blend(lam, bias=extra, want_weights=True)), case
                    differed += not _same(e.blend(lam, gamma=gamma)[1], plain[1])
        e.close()
    g.close()
    assert n < 63 or differed > 0  # gamma matters


# ---- 2. one hypothesis is the handle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 257, 515])
def test_single_member_chain_is_the_handles(hip_mod, n):
    scene = tm._scene("lethal")
    g = tm._scorer(hip_mod, scene)
    e = hip_mod.EnsembleScorer(tm._params(), 0, 1)
    e.load_scene(scene, [scene.agents])
    for K in (1, 4):
        nominal = tm._nominal(K)
        for iterations in (1, 2, 5):
            for gamma in (0.0, 0.3):
                args = (scene.robot_state, n, 7000 + 10 * n + iterations, nominal, tm.SIGMA, tm.WIDE[0], tm.WIDE[1], tm._knot_steps(K),
                        tm.HOLO_GA, iterations, 0.05, gamma)
                stats, plans, best, costs, rejected = e.mppi_run(*args, mode="mean", probs=[1.0], want_costs=True)
                w_stats, w_plans, w_best = g.mppi_run(*args)
                case = (n, K, iterations, gamma)
                assert plans.shape == (iterations, K, 3)
                assert _stat_bits(stats) == _stat_bits(w_stats) and _same(plans, w_plans), case
                assert best == w_best and all(_same(best[f], w_best[f]) for f in ("cost", "vx", "vy", "vtheta")), case
                assert _same(costs, g.costs_view()) and _same(e.member(0).costs_view(), g.costs_view()), case
                assert np.array_equal(rejected, (costs == SFW_COST_INVALID).astype(np.int32)), case
                assert _same(e.knots(0, n), g.knots(0, n)), case
                if n >= 64:
                    assert 0 < stats[-1]["n_valid"] < n, case
    e.close()
    g.close()


# ---- 3. the chain is its defining loop ---------------------------------------------------------------------------------------------
def _loop(e, rs, n, K, seed, nominal, sigma, steps, ga, iterations, lam, gamma, flags, mode, probs):
    """sfw_ensemble_mppi_run's definition, call by call"""
    nom, stats, plans, out = np.array(nominal, dtype=np.float64), [], [], None
    for i in range(iterations):
        out = e.score_perturbed(rs, n, (seed + i) % 2 ** 64, nom, sigma, es.WIDE[0], es.WIDE[1], steps, ga, flags=flags, mode=mode,
                                probs=probs)
        st, u, _ = e.blend([lam], gamma=gamma)
        if st[0]["n_valid"] > 0:
            nom = u[0].copy()
        stats.append(st[0])
        plans.append(nom.copy())
    return stats, np.stack(plans), out[2], out[0], out[1]


def _hold_chain(a, b, scene, n, K, flags, iterations, gamma, mode, probs, seed=None):
    """a runs the chain, b the loop.  Returns what the loop alone showed: (a sample rejected by some hypotheses only, eta > 1 in
    every iteration)."""
    M = a.M
    seed, nominal, sigma, steps, ga = _case(n, K, flags, seed)
    rs = scene.robot_state
    case = (n, K, flags, iterations, gamma, mode, probs)
    stats, plans, best, costs, rejected = a.mppi_run(rs, n, seed, nominal, sigma, es.WIDE[0], es.WIDE[1], steps, ga, iterations, LAM, gamma,
                                                     flags=flags, mode=mode, probs=probs, want_costs=True)
    w_stats, w_plans, w_best, w_costs, w_rejected = _loop(b, rs, n, K, seed, nominal, sigma, steps, ga, iterations, LAM, gamma, flags,
                                                          mode, probs)
    partial = int(np.sum((w_rejected > 0) & (w_rejected < M)))
    print(f"chain {case}: n_valid {[s['n_valid'] for s in w_stats]}, eta {[round(s['eta'], 3) for s in w_stats]}, "
          f"rejected by some {partial}, by all {int(np.sum(w_rejected == M))}")
    # the loop does what an MPPI loop is for (conditions on the scene, not on the code under test)
    assert all(s["n_valid"] > 0 for s in w_stats), case
    if n >= 64:
        steps_ = np.concatenate([np.asarray(nominal)[None], w_plans])
        for i in range(1, iterations):
            assert np.any(_bits(steps_[i]) != _bits(steps_[i + 1])), (case, i)
    # every output
    assert plans.shape == (iterations, K, 3) and np.all(np.isfinite(plans))
    assert _stat_bits(stats) == _stat_bits(w_stats), case
    assert _same(plans, w_plans), case
    assert _same(costs, w_costs) and np.array_equal(rejected, w_rejected), case
    assert best == w_best and all(_same(best[f], w_best[f]) for f in ("cost", "vx", "vy", "vtheta")), case
    # the state: every member, the aggregation, the blend, and what the members were drawn from
    for m in range(M):
        ma, mb = a.member(m), b.member(m)
        assert _same(ma.knots(0, n), mb.knots(0, n)), (case, m)
        if flags & KEEP:
            assert _same(ma.normals(0, n), mb.normals(0, n)), (case, m)
        assert _same(ma.costs_view(), mb.costs_view()) and _same(ma.cost_terms(), mb.cost_terms()), (case, m)
    for md, pr in (("max", None), ("mean", PROBS3[:M] if M == 3 else None), (mode, probs)):
        (ca, ra, ba), (cb, rb, bb) = a.aggregate(md, pr), b.aggregate(md, pr)
        assert _same(ca, cb) and np.array_equal(ra, rb) and ba == bb, (case, md)
    assert _same(ca, costs) and np.array_equal(ra, rejected) and ba == best, case  # (the run's own aggregation again)
    assert _same_blend(a.blend(L16, want_weights=True), b.blend(L16, want_weights=True)), case
    assert _same_blend(a.blend(L16, gamma=0.7), b.blend(L16, gamma=0.7)), case
    if flags & NOMINAL:  # sample 0 of the last iteration is the plan it was drawn around
        before = plans[iterations - 2] if iterations > 1 else nominal
        assert _same(a.knots(0, 1)[:, :, 0], before), case
    return partial > 0, all(s["eta"] > 1.0 for s in w_stats)


# (K, flags, iterations, gamma, mode, probs): every K, flag, iteration count and gamma, both modes, with and without probabilities
CHAINS = [(1, 0, 1, 0.0, "mean", None), (1, 0, 5, 0.3, "max", None), (4, NOMINAL, 2, 0.3, "mean", PROBS3), (4, KEEP, 5, 0.3, "mean", None),
          (4, NO_VY, 2, 0.3, "max", PROBS3), (4, NOMINAL | KEEP, 5, 0.0, "max", None), (1, KEEP, 2, 0.0, "mean", PROBS3),
          (4, 0, 1, 0.3, "mean", None), (1, NO_VY, 5, 0.0, "mean", None)]


@pytest.mark.parametrize("n", [1, 64, 257, 515])
def test_chain_is_the_loop_it_is_defined_by(hip_mod, n):
    scene = es._scene(SCENE)
    hyps = _mixed3(scene)
    a, b = es._ensemble(hip_mod, scene, hyps), es._ensemble(hip_mod, scene, hyps)
    seen = [_hold_chain(a, b, scene, n, *c) for c in CHAINS]
    a.close()
    b.close()
    if n >= 257:  # 4. not vacuous
        assert any(p for p, _ in seen), "no parametrisation has a sample rejected by some hypotheses only"
        assert any(e for _, e in seen), "no parametrisation has eta > 1 in every iteration"


def test_chain_on_every_scoring_path(hip_mod, monkeypatch):
    scene = es._scene(SCENE)
    hyps = _mixed3(scene)
    ref = es._ensemble(hip_mod, scene, hyps)
    monkeypatch.setenv("SFW_CYCLE_FUSED", "0")
    unfused = es._ensemble(hip_mod, scene, hyps)
    _hold_chain(unfused, ref, scene, 64, 4, NOMINAL, 2, 0.3, "mean", None)
    assert unfused.member(0).plan_info()["one_launch"] == 0
    monkeypatch.delenv("SFW_CYCLE_FUSED")
    monkeypatch.setenv("SFW_TABLE_BUDGET_MB", "1")
    chunked = es._ensemble(hip_mod, scene, hyps)
    monkeypatch.delenv("SFW_TABLE_BUDGET_MB")
    _hold_chain(chunked, ref, scene, 2100, 4, 0, 2, 0.3, "max", None)
    assert chunked.member(0).plan_info()["chunks"] > 1
    monkeypatch.setenv("SFW_DEVICE_CUS", "32")
    small = es._ensemble(hip_mod, scene, hyps)
    monkeypatch.delenv("SFW_DEVICE_CUS")
    _hold_chain(small, ref, scene, 2100, 4, KEEP, 2, 0.3, "mean", PROBS3)
    _hold_chain(small, ref, scene, 515, 1, 0, 5, 0.3, "mean", None)
    for e in (ref, unfused, chunked, small):
        e.close()


def test_seeds_near_the_top_and_repeats(hip_mod):
    scene = es._scene("cfg2_8")  # (8 people: the members do not take the one-launch cycle)
    hyps = _mixed3(scene)
    a, b = es._ensemble(hip_mod, scene, hyps), es._ensemble(hip_mod, scene, hyps)
    for seed in (2 ** 64 - 2, 5):  # seed + i wraps modulo 2^64
        _hold_chain(a, b, scene, 130, 3, 0, 4, 0.3, "mean", None, seed=seed)
    # repeating the call gives the same bits, also after another size has grown the buffers
    seed, nominal, sigma, steps, ga = _case(130, 3, 0)
    args = (scene.robot_state, 130, seed, nominal, sigma, es.WIDE[0], es.WIDE[1], steps, ga, 3, LAM, 0.3)
    first = a.mppi_run(*args, want_costs=True)
    a.mppi_run(scene.robot_state, 2100, 9, es._nominal(8), es.SIGMA, es.WIDE[0], es.WIDE[1], tuple(range(8)), es.HOLO_GA, 8, LAM, 0.3)
    again = a.mppi_run(*args, want_costs=True)
    assert _stat_bits(again[0]) == _stat_bits(first[0]) and _same(again[1], first[1]) and again[2] == first[2]
    assert _same(again[3], first[3]) and np.array_equal(again[4], first[4])
    # the last iteration is a perturbed score like any other: score_perturbed with its seed and nominal scores the same
    c, r, bst = a.score_perturbed(scene.robot_state, 130, seed + 2, first[1][1], sigma, es.WIDE[0], es.WIDE[1], steps, ga)
    assert _same(c, first[3]) and np.array_equal(r, first[4]) and bst == first[2]
    a.close()
    b.close()


# ---- 5. no valid rollout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [45, 257])
def test_no_valid_rollout_keeps_the_nominal(hip_mod, n):
    """the blocked scene, and in ONE of three hypotheses a person standing on the robot: every rollout is rejected"""
    fx = gu.Fixture("blocked")
    e = hip_mod.EnsembleScorer(fx.params(), 0, 3)
    e.set_costmap(fx.cells, fx.origin_x, fx.origin_y, fx.resolution)
    e.set_footprint(fx.footprint)
    on_robot = es._with_person(fx.agents, fx.robot_state[0] + 0.1, fx.robot_state[1], 0.0, 0.0)
    for m in range(3):
        e.set_hypothesis(m, on_robot if m == 1 else fx.agents, fx.obstacles)
    nominal = tm._nominal(3)
    ga = (fx.goal_args[0], 1.0) + tuple(fx.goal_args[2:])
    for gamma in (0.0, 0.3):
        stats, plans, best, costs, rejected = e.mppi_run(fx.robot_state, n, 3, nominal, tm.SIGMA, tm.WIDE[0], tm.WIDE[1], (0, 2, 5), ga, 3,
                                                         0.5, gamma, mode="mean", want_costs=True)  # (raises unless SFW_OK)
        assert np.all(costs == SFW_COST_INVALID) and np.all(rejected >= 1)
        for s in stats:
            assert (s["lambda"], s["j_min"], s["eta"], s["sum_w2"], s["n_valid"], s["index_min"]) == (0.5, -1.0, 0.0, 0.0, 0, -1)
            assert _bits(s["eta"]).item() == 0 and _bits(s["sum_w2"]).item() == 0
        for i in range(3):
            assert _same(plans[i], nominal)
        assert best["index"] == -1 and best["n_valid"] == 0
    e.close()


# ---- 6. refusals and state ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_score_usable(hip_mod):
    scene = es._scene(SCENE)
    e = es._ensemble(hip_mod, scene, _mixed3(scene))
    n, K = 65, 3
    seed, nominal, sigma, steps, ga = _case(n, K, 0)
    rs = scene.robot_state
    ref_score = e.score_perturbed(rs, n, seed, nominal, sigma, es.WIDE[0], es.WIDE[1], steps, ga)
    ref_blend, ref_ctrl = e.blend(L16, want_weights=True), e.blend(L16, gamma=0.3, want_weights=True)
    L = hip_mod.lib()
    keep = []

    def unchanged(what):
        c, r, b = e.aggregate("mean")
        assert _same(c, ref_score[0]) and np.array_equal(r, ref_score[1]) and b == ref_score[2], what
        assert _same_blend(e.blend(L16, want_weights=True), ref_blend), what
        assert _same_blend(e.blend(L16, gamma=0.3, want_weights=True), ref_ctrl), what
        for m in range(e.M):  # nothing half-staged: every member still holds the launch of the score
            assert _same(e.member(m).costs_view(), e.member(m).fetch()[0]), (what, m)

    def perturb_of(nominal=nominal, sigma=sigma, lo=es.WIDE[0], hi=es.WIDE[1], flags=0, reserved=0, null_nominal=False):
        p, nom, _ = hip_mod.HipScorer._perturb(3, nominal, sigma, lo, hi, steps, flags)
        keep.append(nom)
        p.reserved = reserved
        if null_nominal:
            p.nominal = None
        return p

    stat, plans, sel = (SfwBlendStat * 32)(), np.zeros((32, K, 3)), SfwBest()
    costs, rej = np.zeros(n), np.zeros(n, dtype=np.int32)

    def run(p=None, m=(2, 0, 0.5, 0.3), rs_=rs, n_=n, K_=K, steps_=steps, ga_=ga, mode=0, probs=None, null_p=False, null_m=False,
            stat_p=stat, plans_p=plans.ctypes.data):
        p = perturb_of() if p is None else p
        mm = SfwMppi(*m)
        ks = None if steps_ is None else np.ascontiguousarray(steps_, dtype=np.int32)
        pr = None if probs is None else np.ascontiguousarray(probs, dtype=np.float64)
        return L.sfw_ensemble_mppi_run(e._e, None if rs_ is None else C.byref(SfwRobotState(*rs_)), None if null_p else C.byref(p), n_, K_,
                                       es._ptr(ks), None if ga_ is None else C.byref(SfwGoalArgs(*ga_)), mode, es._ptr(pr),
                                       None if null_m else C.byref(mm), stat_p, plans_p, costs.ctypes.data, rej.ctypes.data, C.byref(sel))

    nan_nominal = np.array(nominal)
    nan_nominal[1, 2] = np.nan
    refused = [
        # 1. mode and probabilities
        lambda: run(mode=7), lambda: run(mode=2), lambda: run(probs=[0.5, -0.1, 0.6]), lambda: run(probs=[np.nan] * 3),
        # 2. m
        lambda: run(null_m=True), lambda: run(m=(0, 0, 0.5, 0.3)), lambda: run(m=(-1, 0, 0.5, 0.3)), lambda: run(m=(33, 0, 0.5, 0.3)),
        lambda: run(m=(2, 1, 0.5, 0.3)), lambda: run(m=(2, 0, 0.0, 0.3)), lambda: run(m=(2, 0, -0.5, 0.3)),
        lambda: run(m=(2, 0, np.nan, 0.3)), lambda: run(m=(2, 0, np.inf, 0.3)), lambda: run(m=(2, 0, 0.5, np.nan)),
        lambda: run(m=(2, 0, 0.5, np.inf)), lambda: run(m=(2, 0, 0.5, -np.inf)),
        # 3. the outputs that are not optional
        lambda: run(stat_p=None), lambda: run(plans_p=None),
        # 4. what sfw_ensemble_score_perturbed refuses
        lambda: run(null_p=True), lambda: run(perturb_of(null_nominal=True)), lambda: run(rs_=None), lambda: run(ga_=None),
        lambda: run(steps_=None), lambda: run(n_=0), lambda: run(K_=0), lambda: run(K_=65), lambda: run(steps_=(2, 9, 23)),
        lambda: run(steps_=(0, 9, 9)), lambda: run(perturb_of(flags=8)), lambda: run(perturb_of(reserved=1)),
        lambda: run(perturb_of(nominal=nan_nominal)), lambda: run(perturb_of(sigma=(0.1, -0.1, 0.1))),
        lambda: run(perturb_of(lo=(0.0, 0.0, 0.6), hi=(0.7, 0.3, 0.5))), lambda: run(perturb_of(flags=NO_VY)),
        lambda: run(rs_=(0.0, np.nan, 0.0, 0.3, 0.0, 0.0)), lambda: run(ga_=(6.0, 3.0, np.inf, 2.0, 0.5)),
    ]
    for i, call in enumerate(refused):
        assert call() == SFW_ERR_INVALID_ARG, i
        unchanged(i)
    assert not np.any(plans) and stat[0].n_valid == 0 and not np.any(costs)  # a refused call writes nothing
    # the order: an earlier rule answers first — here each call breaks two, and only a later one would leave the message
    assert run(mode=7, null_m=True) == SFW_ERR_INVALID_ARG and "mode" in str(L.sfw_ensemble_last_error(e._e))
    assert run(null_m=True, stat_p=None) == SFW_ERR_INVALID_ARG and "m is NULL" in str(L.sfw_ensemble_last_error(e._e))
    assert run(stat_p=None, n_=0) == SFW_ERR_INVALID_ARG and "stat_out" in str(L.sfw_ensemble_last_error(e._e))
    # blend_control's own refusals
    lam, u = np.array([0.5]), np.zeros((16, K, 3))
    nan_bias = np.zeros(n)
    nan_bias[n - 1] = np.nan
    bc = L.sfw_ensemble_blend_control
    refused = [bc(e._e, None, 1, 0.5, None, stat, u.ctypes.data, None), bc(e._e, lam.ctypes.data, 0, 0.5, None, stat, u.ctypes.data, None),
               bc(e._e, lam.ctypes.data, 17, 0.5, None, stat, u.ctypes.data, None), bc(e._e, lam.ctypes.data, 1, np.nan, None, stat, u.ctypes.data, None),
               bc(e._e, lam.ctypes.data, 1, -np.inf, None, stat, u.ctypes.data, None), bc(e._e, lam.ctypes.data, 1, 0.5, None, None, u.ctypes.data, None),
               bc(e._e, lam.ctypes.data, 1, 0.5, None, stat, None, None), bc(e._e, np.array([-1.0]).ctypes.data, 1, 0.5, None, stat, u.ctypes.data, None),
               bc(e._e, lam.ctypes.data, 1, 0.5, nan_bias.ctypes.data, stat, u.ctypes.data, None)]
    assert refused == [SFW_ERR_INVALID_ARG] * len(refused), refused
    unchanged("blend_control")
    # the limits themselves are accepted
    assert run(m=(32, 0, 1e-9, -1e6)) == SFW_OK and run(m=(1, 0, 1e9, 0.0)) == SFW_OK
    e.close()


def test_state_rules(hip_mod):
    scene = es._scene(SCENE)
    hyps = _mixed3(scene)
    rs = scene.robot_state
    n, K = 65, 3
    seed, nominal, sigma, steps, ga = _case(n, K, 0)
    run_args = (rs, n, seed, nominal, sigma, es.WIDE[0], es.WIDE[1], steps, ga, 3, LAM, 0.3)

    def state_error(call, text=None):
        with pytest.raises(hip_mod.SfwError) as ex:
            call()
        assert ex.value.status == SFW_ERR_STATE and (text is None or text in str(ex.value)), str(ex.value)

    # a hypothesis never set; nothing scored
    e = hip_mod.EnsembleScorer(es._params(scene), 0, 3)
    e.set_costmap(scene.cells, scene.origin_x, scene.origin_y, scene.resolution)
    e.set_footprint(scene.footprint)
    e.set_hypothesis(0, *hyps[0])
    e.set_hypothesis(2, *hyps[2])
    state_error(lambda: e.mppi_run(*run_args), "hypothesis 1")
    state_error(lambda: e.blend([1.0], gamma=0.3))
    e.set_hypothesis(1, *hyps[1])
    # the control cost needs a perturbed score: not host-staged sequences, not a grid
    es._score(e, scene, es._case(n, K))
    state_error(lambda: e.blend([1.0], gamma=0.3), "perturbed")
    e.blend([1.0])  # (the plain blend serves them)
    e.score_grid(rs, scene.linvels, scene.angvels, scene.goal_args)
    state_error(lambda: e.blend([1.0], gamma=0.3), "perturbed")
    e.blend([1.0])
    # after a run: member 0's own blend with the control cost and the ensemble's do not disturb each other
    stats, plans, best = e.mppi_run(*run_args)
    ref = e.blend(L16, gamma=0.3, want_weights=True)
    m0 = e.member(0)
    own = m0.blend(L16, gamma=0.7, want_weights=True)
    assert not _same(own[1], ref[1])  # (its own cost vector and another gamma: another result)
    assert _same_blend(e.blend(L16, gamma=0.3, want_weights=True), ref)
    assert _same_blend(m0.blend(L16, gamma=0.7, want_weights=True), own)
    assert _same_blend(e.blend(L16, gamma=0.3, want_weights=True), ref)
    own_cc = m0.control_cost(0.7)
    e.blend(L16, gamma=0.3, bias=np.ones(n))
    assert _same(m0.control_cost(0.7), own_cc) and _same_blend(m0.blend(L16, gamma=0.7, want_weights=True), own)
    # a member touched since the run
    vx, vy, vth, ksteps, cga = es._case(n, K)
    e.member(1).stage_sequences(rs, vx, vth, ksteps, cga, vy=vy)
    for call in (lambda: e.blend([1.0], gamma=0.3), lambda: e.blend([1.0]), lambda: e.aggregate("mean")):
        state_error(call, "member 1")
    s2, p2, b2 = e.mppi_run(*run_args)  # ... and the next run stages it again
    assert _stat_bits(s2) == _stat_bits(stats) and _same(p2, plans) and b2 == best
    e.member(2).score_one(rs, 0.3, 0.0, 0.1, scene.goal_args)
    state_error(lambda: e.blend([1.0], gamma=0.3), "member 2")
    # parameters changed through a member
    e.member(1).set_params(es._params(scene, social_weight=2.0))
    state_error(lambda: e.mppi_run(*run_args))
    e.set_params(es._params(scene))
    s3, p3, b3 = e.mppi_run(*run_args)
    assert _stat_bits(s3) == _stat_bits(stats) and _same(p3, plans) and b3 == best
    us = e.last_us()
    assert us["stage"] > 0 and us["enqueue"] > 0 and us["wait_fetch"] > 0
    e.close()  # destroy after a run
    for _ in range(3):  # ... and with nothing else done on the ensemble
        e = es._ensemble(hip_mod, scene, hyps)
        s4, p4, b4 = e.mppi_run(*run_args)
        e.close()
        assert _stat_bits(s4) == _stat_bits(stats) and _same(p4, plans) and b4 == best
