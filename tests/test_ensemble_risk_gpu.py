"""sfw_ensemble_set_risk on the device: the tail expectation of the social work and the bound on the contact mass, held to
"Risk" in include/sfw_hip.h through its numpy restatement (social_force_window_planner_amd/risk.py) fed the members' own
captured terms.  Everything is compared bitwise (uint64 views): no tolerance appears.

Shapes (the smallest that reach every path): the reference's 5 x 9 grid (45 samples: one block that writes the record itself,
the members' one-launch cycle, a skipped sample), the cfg2 variant cut to 48 x 48 with 8 people (9 blocks and the second
stage), a list of n = 515 with K = 3 (a ragged last block), the six mixed hypotheses of tests/test_ensemble_gpu.py, and M = 64
on the 5 x 9 grid with tail_mass = 1 and unequal probabilities (the longest walk).

The contact-mass scene (CONTACT_PEOPLE) gives every member one more person of its own: three head-on at different offsets, one
walking away.  On the CPU oracle that leaves, on the 5 x 9 grid, 2 / 3 / 2 samples rejected by one / two / three of the four
members, member 0 among the rejecting ones in all of the last two kinds; on the 48 x 48 grid 149 / 44 / 13, member 0 rejecting
in 3 / 44 / 13 of them.  The test asserts that mix on the device's own results and fails, not skips, without it."""
import ctypes as C

import numpy as np
import pytest

import test_ensemble_gpu as eg
import test_ensemble_mppi_gpu as em
import test_ensemble_sequences_gpu as es
from social_force_window_planner_amd import risk
from social_force_window_planner_amd._abi import (SFW_COST_INVALID, SFW_COST_SKIPPED, SFW_ERR_INVALID_ARG, SFW_ERR_STATE,
                                                   SFW_PRECISION_F32, SFW_PRECISION_F64, SfwRisk)
from social_force_window_planner_amd.hypotheses import naive_goal_hypotheses
from sfw_test_util import _bits, _np_best, _same, _scene_params as _params

pytestmark = pytest.mark.gpu

GRIDS = eg.GRIDS
TAILS = (1.0, 0.5, 0.3, 1.0 / 6.0, 0.05)
CONTACTS = (0.0, 0.2)
PROBS6 = [0.5, 0.1, 0.0, 0.1, 0.15, 0.3]  # unequal, one zero
CONTACT_PEOPLE = [(1.8, 0.1, -1.3, 0.0), (1.6, 0.1, 1.3, 0.0), (1.5, 0.6, -1.0, -0.3), (1.8, 0.0, -1.0, 0.0)]


def _restated(e, params, mode, probs, tail_mass, contact_mass):
    terms = [e.member(m).cost_terms() for m in range(e.M)]
    return risk.ensemble_risk(terms, eg._weights(params), mode, probs, tail_mass=tail_mass, contact_mass=contact_mass)


def _hold_grid(oracle_mod, scene, got, want, what):
    (costs, rejected, best), (hc, hr) = got, want
    assert np.array_equal(rejected, hr), what
    assert _same(costs, hc), f"{what}: {int(np.sum(_bits(costs) != _bits(hc)))} costs differ"
    assert best == oracle_mod.select_best(scene.linvels, scene.angvels, hc), what
    assert best["n_valid"] == int(np.sum(hc >= 0)), what


# ---- 1. no risk, or a risk cleared: the plain aggregation -----------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_without_a_risk_nothing_changes(hip_mod, grid):
    scene = eg._scene(grid)
    hyps = eg._mixed_hypotheses(scene)
    plain, e = eg._ensemble(hip_mod, scene, hyps), eg._ensemble(hip_mod, scene, hyps)
    assert e.risk() is None
    e.set_risk(0.3, 0.2)
    assert e.risk() == {"tail_mass": 0.3, "contact_mass": 0.2}
    under = e.score_grid(*eg._grid_args(scene), mode="mean", probs=PROBS6)
    e.clear_risk()
    assert e.risk() is None
    differed = False
    for mode in ("mean", "max"):
        for probs in (None, PROBS6):
            want = plain.score_grid(*eg._grid_args(scene), mode=mode, probs=probs)
            for got in (e.aggregate(mode, probs), e.score_grid(*eg._grid_args(scene), mode=mode, probs=probs)):
                assert _same(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (mode, probs)
            differed |= mode == "mean" and probs is not None and not _same(under[0], want[0])
    assert differed, "the risk that was cleared had changed nothing"
    plain.close()
    e.close()


# ---- 2. the definition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("probs", [None, PROBS6])
def test_mixed_hypotheses_match_the_definition(hip_mod, oracle_mod, grid, probs):
    scene = eg._scene(grid)
    p = _params(scene)
    e = eg._ensemble(hip_mod, scene, eg._mixed_hypotheses(scene), p)
    seen = {}
    for contact in CONTACTS:
        for mode in ("mean", "max"):
            for i, tail in enumerate(TAILS if mode == "mean" else TAILS[2:3]):  # (MAX does not read tail_mass)
                e.set_risk(tail, contact)
                got = e.score_grid(*eg._grid_args(scene), mode=mode, probs=probs) if i == 0 else e.aggregate(mode, probs)
                want = _restated(e, p, mode, probs, tail, contact)
                _hold_grid(oracle_mod, scene, got, want, (mode, tail, contact))
                seen[mode, tail, contact] = got[0]
    for contact in CONTACTS:  # the tail mass is read
        assert not _same(seen["mean", TAILS[0], contact], seen["mean", TAILS[-1], contact]), "the whole mass and its worst 5 % cost the same"
    # (on these grids the six hypotheses reject together: what contact_mass admits is test_contact_mass_admits_what_few_members_reject's)
    assert np.any(got[0] == SFW_COST_SKIPPED) == (grid == "ref5x9")
    e.close()


def test_sixty_four_members(hip_mod, oracle_mod):
    scene = eg._scene("ref5x9")
    p = _params(scene)
    hyps = naive_goal_hypotheses(scene.agents, tuple(0.5 * k for k in range(1, 9)), tuple(0.2 * k - 0.7 for k in range(8)))
    assert len(hyps) == 64
    e = eg._ensemble(hip_mod, scene, [(h, scene.obstacles) for h in hyps], p)
    probs = [(1 + (7 * m) % 13) / 100.0 for m in range(64)]
    e.set_risk(1.0, 0.0)
    got = e.score_grid(*eg._grid_args(scene), mode="mean", probs=probs)
    _hold_grid(oracle_mod, scene, got, _restated(e, p, "mean", probs, 1.0, 0.0), "M = 64")
    assert got[2]["n_valid"] > 0
    W = np.stack([e.member(m).cost_terms()[:, 4] for m in range(64)])[:, got[0] >= 0]
    assert np.all((W.max(axis=0) - W.min(axis=0)) > 0), "the members' social work does not differ: nothing to order"
    e.set_risk(0.3, 0.1)
    _hold_grid(oracle_mod, scene, e.aggregate("mean", probs), _restated(e, p, "mean", probs, 0.3, 0.1), "M = 64, tail 0.3")
    e.close()


# ---- 3. M = 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("precision", [SFW_PRECISION_F64, SFW_PRECISION_F32])
def test_single_member_is_the_standalone_handle(hip_mod, grid, precision):
    scene = eg._scene(grid)
    p = _params(scene, precision)
    e = eg._ensemble(hip_mod, scene, [(scene.agents, scene.obstacles)], p)
    e.set_risk(1.0, 0.0)
    g = eg._standalone(hip_mod, scene, scene.agents, scene.obstacles, p)
    gc, gb = g.score_grid(*eg._grid_args(scene))
    for mode in ("mean", "max"):
        costs, rejected, best = e.score_grid(*eg._grid_args(scene), mode=mode, probs=[1.0])
        assert _same(costs, gc), f"{int(np.sum(_bits(costs) != _bits(gc)))} costs differ"
        assert best == gb and np.array_equal(rejected, (gc == SFW_COST_INVALID).astype(np.int32))
    assert np.any(gc >= 0)
    e.close()
    g.close()


# ---- 4. the contact mass --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_contact_mass_admits_what_few_members_reject(hip_mod, oracle_mod, grid):
    scene = eg._scene(grid)
    p = _params(scene)
    M = len(CONTACT_PEOPLE)
    e = eg._ensemble(hip_mod, scene, [(eg._with_person(scene.agents, *q), scene.obstacles) for q in CONTACT_PEOPLE], p)
    e.set_risk(0.5, 0.0)
    strict = e.score_grid(*eg._grid_args(scene), mode="mean")
    rejected = strict[1]
    by_member_0 = np.stack([e.member(m).cost_terms()[:, 1] for m in range(M)])[0] == SFW_COST_INVALID
    partial = (rejected > 0) & (rejected < M)
    few, many = partial & (rejected <= M // 2), partial & (rejected > M // 2)
    print(f"{grid}: rejected by 1..{M - 1} members: {[int(np.sum(rejected == k)) for k in range(1, M)]}, member 0 among them "
          f"{[int(np.sum((rejected == k) & by_member_0)) for k in range(1, M)]}")
    assert few.any() and many.any() and np.any(few & by_member_0), "the scene holds no sample of the kinds this test is about"
    _hold_grid(oracle_mod, scene, strict, _restated(e, p, "mean", None, 0.5, 0.0), "contact_mass 0")
    assert np.all(strict[0][partial] == SFW_COST_INVALID)
    for mode in ("mean", "max"):
        e.set_risk(0.5, 0.5)
        got = e.aggregate(mode)
        _hold_grid(oracle_mod, scene, got, _restated(e, p, mode, None, 0.5, 0.5), f"contact_mass 0.5, {mode}")
        assert np.array_equal(got[1], rejected)
        assert np.all(got[0][few] >= 0) and np.all(got[0][many] == SFW_COST_INVALID)
        assert got[2]["n_valid"] == strict[2]["n_valid"] + int(few.sum())
        e.set_risk(0.5, 0.0)
        back = e.aggregate(mode)
        assert np.all(back[0][partial] == SFW_COST_INVALID) and back[2]["n_valid"] == strict[2]["n_valid"]
    # unequal probabilities: member 0 (0.1) alone stays within contact_mass = 0.2, members 0 and 3 (0.3) do not
    probs = [0.1, 0.4, 0.3, 0.2]
    for contact in (0.2, 0.5):
        for mode, tail in (("mean", 1.0), ("mean", 0.3), ("max", 1.0)):
            e.set_risk(tail, contact)
            _hold_grid(oracle_mod, scene, e.aggregate(mode, probs), _restated(e, p, mode, probs, tail, contact), (mode, tail, contact))
    e.close()


# ---- 5. re-aggregation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_set_risk_then_aggregate_is_a_fresh_score(hip_mod, grid):
    scene = eg._scene(grid)
    hyps = eg._mixed_hypotheses(scene)
    e, fresh = eg._ensemble(hip_mod, scene, hyps), eg._ensemble(hip_mod, scene, hyps)
    e.set_risk(0.5, 0.2)
    with pytest.raises(hip_mod.SfwError) as ex:
        e.aggregate("mean")
    assert ex.value.status == SFW_ERR_STATE  # nothing scored
    e.clear_risk()
    e.score_grid(*eg._grid_args(scene), mode="max")
    for tail in TAILS:  # the sweep: no stage in between
        e.set_risk(tail, 0.2)
        fresh.set_risk(tail, 0.2)
        got, want = e.aggregate("mean", PROBS6), fresh.score_grid(*eg._grid_args(scene), mode="mean", probs=PROBS6)
        assert _same(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], tail
    # the state rules of sfw_ensemble_aggregate are unchanged
    e.member(1).stage(*eg._grid_args(scene))
    with pytest.raises(hip_mod.SfwError) as ex:
        e.aggregate("mean")
    assert ex.value.status == SFW_ERR_STATE and "member 1" in str(ex.value)
    e.score_grid(*eg._grid_args(scene))
    e.member(0).score_one(scene.robot_state, 0.3, 0.0, 0.1, scene.goal_args)
    with pytest.raises(hip_mod.SfwError) as ex:
        e.aggregate("max")
    assert ex.value.status == SFW_ERR_STATE
    e.close()
    fresh.close()


# ---- 6. the list form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene_name", es.SCENES)
def test_sequences_and_perturbed_under_a_risk(hip_mod, scene_name):
    scene = es._scene(scene_name)
    hyps = es._mixed_hypotheses(scene)
    M, n, K = len(hyps), 515, 3
    p = _params(scene)
    e = es._ensemble(hip_mod, scene, hyps, p)
    case = es._case(n, K)
    vx, vy, vth = case[:3]
    plain = es._score(e, scene, case, mode="mean", probs=PROBS6)
    es._hold_mix(plain[1], M, n, "risk list")
    relaxed = 0
    for mode, tail, contact in (("mean", 0.3, 0.2), ("mean", 1.0, 0.0), ("max", 0.5, 0.2)):
        e.set_risk(tail, contact)
        costs, rejected, best = es._score(e, scene, case, mode=mode, probs=PROBS6)
        hc, hr = _restated(e, p, mode, PROBS6, tail, contact)
        assert np.array_equal(rejected, hr) and np.array_equal(rejected, plain[1])
        assert _same(costs, hc), f"{mode}: {int(np.sum(_bits(costs) != _bits(hc)))} costs differ"
        assert best == _np_best(hc, vx[0], None if vy is None else vy[0], vth[0])
        assert best["n_valid"] == int(np.sum(hc >= 0))
        relaxed += int(np.sum((rejected > 0) & (costs >= 0)))
        ac, ar, ab = e.aggregate(mode, PROBS6)
        assert _same(ac, costs) and np.array_equal(ar, rejected) and ab == best
        # the blend reads this cost vector, as tests/test_ensemble_sequences_gpu.py holds it for the plain modes
        knots = es._knots(vx, vy, vth)
        for lambdas, bias in es._blends(n)[1:3]:
            got = e.blend(lambdas, bias=bias, want_weights=True)
            assert all(s["n_valid"] == best["n_valid"] for s in got[0])
            es._hold_weights(costs, lambdas, bias, got[0], got[2])
            es._hold_to_mirror(costs, knots, lambdas, bias, got)
    assert relaxed > 0, "no sample rejected by some hypotheses became valid"
    # perturbed: the same restatement over the knots the device drew, and the same results as those knots handed over
    seed, nominal, sigma, steps, ga = es._perturbed_case(scene_name, n, K, 0)
    e.set_risk(0.3, 0.2)
    costs, rejected, best = e.score_perturbed(scene.robot_state, n, seed, nominal, sigma, es.WIDE[0], es.WIDE[1], steps, ga, mode="mean",
                                              probs=PROBS6)
    hc, hr = _restated(e, p, "mean", PROBS6, 0.3, 0.2)
    assert np.array_equal(rejected, hr) and _same(costs, hc)
    es._hold_mix(rejected, M, n, "risk perturbed")
    u = e.knots(0, n)
    assert best == _np_best(hc, u[0, 0], u[0, 1], u[0, 2])
    sc, sr, sb = e.score_sequences(scene.robot_state, u[:, 0, :], u[:, 2, :], steps, ga, vy=u[:, 1, :], mode="mean", probs=PROBS6)
    assert _same(costs, sc) and np.array_equal(rejected, sr) and best == sb
    got = e.blend(es.L16, want_weights=True)
    es._hold_weights(sc, es.L16, None, got[0], got[2])
    es._hold_to_mirror(sc, u, es.L16, None, got)
    e.close()


# ---- 7. the chain ---------------------------------------------------------------------------------------------------------------
def test_chain_under_a_risk_is_its_defining_loop(hip_mod):
    scene = es._scene(em.SCENE)
    hyps = em._mixed3(scene)
    a, b = es._ensemble(hip_mod, scene, hyps), es._ensemble(hip_mod, scene, hyps)
    seed, nominal, sigma, steps, ga = em._case(515, 3, 0)
    args = (scene.robot_state, 515, seed, nominal, sigma, es.WIDE[0], es.WIDE[1], steps, ga, 3, em.LAM, 0.3)
    plain = a.mppi_run(*args, mode="mean", probs=em.PROBS3, want_costs=True)
    seen = []
    for tail, contact, mode, probs in ((0.4, 0.45, "mean", em.PROBS3), (1.0, 0.0, "mean", None), (0.4, 0.45, "max", em.PROBS3)):
        a.set_risk(tail, contact)
        b.set_risk(tail, contact)
        seen.append(em._hold_chain(a, b, scene, 515, 3, 0, 3, 0.3, mode, probs))
    assert any(p for p, _ in seen), "no sample rejected by some hypotheses only"
    # the risk took part in the chain: its plans are not the plain chain's
    a.set_risk(0.4, 0.45)
    under = a.mppi_run(*args, mode="mean", probs=em.PROBS3, want_costs=True)
    assert not _same(under[1], plain[1]) and not _same(under[3], plain[3])
    a.close()
    b.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(hip_mod):
    scene = eg._scene("ref5x9")
    hyps = eg._mixed_hypotheses(scene)
    M = len(hyps)
    e = eg._ensemble(hip_mod, scene, hyps)
    nan, inf = float("nan"), float("inf")
    e.set_risk(0.25, 0.125)
    ref = e.score_grid(*eg._grid_args(scene), mode="mean", probs=PROBS6)
    for tail, contact in ((0.0, 0.1), (-0.5, 0.1), (1.0000001, 0.1), (nan, 0.1), (inf, 0.1), (0.5, -1e-9), (0.5, 1.0), (0.5, 1.5),
                          (0.5, nan), (0.5, inf), (-inf, 0.0)):
        with pytest.raises(hip_mod.SfwError) as ex:
            e.set_risk(tail, contact)
        assert ex.value.status == SFW_ERR_INVALID_ARG, (tail, contact)
        assert e.risk() == {"tail_mass": 0.25, "contact_mass": 0.125}
    L = hip_mod.lib()
    for reserved in (1, -1, 1 << 40):
        assert L.sfw_ensemble_set_risk(e._e, C.byref(SfwRisk(0.5, 0.0, reserved))) == SFW_ERR_INVALID_ARG
        assert e.risk() == {"tail_mass": 0.25, "contact_mass": 0.125}
    assert L.sfw_ensemble_get_risk(e._e, None, None) == SFW_ERR_INVALID_ARG
    # the edges of the ranges are accepted
    for tail, contact in ((1.0, 0.0), (5e-324, 0.0), (0.5, 1.0 - 2.0 ** -53)):
        e.set_risk(tail, contact)
        assert e.risk() == {"tail_mass": tail, "contact_mass": contact}
    e.set_risk(0.25, 0.125)
    # all-zero probabilities under a risk: refused before any stage, by every aggregating call; the previous score stays usable
    zeros = [0.0] * M
    seed, nominal, sigma, steps, ga = es._perturbed_case("ref5x9", 65, 3, 0)
    vx, vy, vth, ksteps, kga = es._case(65, 3)
    calls = (lambda: e.score_grid(*eg._grid_args(scene), mode="mean", probs=zeros),
             lambda: e.score_sequences(scene.robot_state, vx, vth, ksteps, kga, vy=vy, mode="max", probs=zeros),
             lambda: e.score_perturbed(scene.robot_state, 65, seed, nominal, sigma, es.WIDE[0], es.WIDE[1], steps, ga, mode="mean",
                                       probs=zeros),
             lambda: e.mppi_run(scene.robot_state, 65, seed, nominal, sigma, es.WIDE[0], es.WIDE[1], steps, ga, 2, 1.0, 0.3,
                                mode="mean", probs=zeros),
             lambda: e.aggregate("mean", zeros))
    for i, call in enumerate(calls):
        with pytest.raises(hip_mod.SfwError) as ex:
            call()
        assert ex.value.status == SFW_ERR_INVALID_ARG and "zero" in str(ex.value), i
        got = e.aggregate("mean", PROBS6)
        assert _same(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2], i
    # without a risk all-zero probabilities stay what they were: accepted
    e.clear_risk()
    c, _, _ = e.aggregate("mean", zeros)
    assert len(c) == len(ref[0])
    # mode keeps its two values
    e.set_risk(0.25, 0.125)
    for mode in (2, 7):
        with pytest.raises(hip_mod.SfwError) as ex:
            e.aggregate(mode)
        assert ex.value.status == SFW_ERR_INVALID_ARG
    e.close()
