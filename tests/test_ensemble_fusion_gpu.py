"""sfw_ensemble_set_list_fusion: the M members of an ensemble scored in one batched launch instead of M.

Two ensembles with the same hypotheses, one with the switch on and one with it off (the parent's path), are held bitwise equal
(uint64 views) in everything sfw_ensemble_score_sequences, _score_perturbed and _mppi_run return and leave behind: records,
plans, ensemble costs, `rejected`, the winner; every member's costs, terms, knots and normals; and what aggregate() and blend()
make of it afterwards.  The scenes are those of tests/test_batch_lists_gpu.py (5 x 5 m, 12 steps)."""
import numpy as np
import pytest

import test_batch_lists_gpu as bl
from social_force_window_planner_amd._abi import SFW_PERTURB_KEEP_NORMALS, SfwAgent
from social_force_window_planner_amd.hypotheses import naive_goal_hypotheses
from sfw_test_util import _bits, _nominal, _same
from test_ensemble_sequences_gpu import _laser, _with_person

pytestmark = pytest.mark.gpu

KEEP = SFW_PERTURB_KEEP_NORMALS
L4 = bl.L4
STEPS = (0, 2, 7)
ITER = 3


def _hypotheses(M):
    """crowds of different sizes, one of them empty; hypothesis 7 of 8 has laser points (another kernel variant)"""
    scene = bl._scene(5, 305)
    naive = [(h, scene.obstacles) for h in naive_goal_hypotheses(scene.agents, (1.0, 3.0), (0.0, 0.5))]
    empty = ((SfwAgent * 1)(scene.agents[0]), scene.obstacles)
    more = (_with_person(scene.agents, 1.5, -0.6, -0.3, 0.6), scene.obstacles)
    laser = (naive_goal_hypotheses(scene.agents, (2.0,))[0], _laser(60))
    pool = [naive[0], empty, more, naive[1], naive[2], naive[3], naive[0], laser]
    return scene, ([pool[m % 7] for m in range(M)] if M > 8 else pool[:M])


def _pair(hip_mod, M):
    scene, hyps = _hypotheses(M)
    out = []
    for fusion in (True, False):
        e = hip_mod.EnsembleScorer(bl._params(), 0, M)
        e.load_scene(scene, hyps)
        assert e.list_fusion() == 0
        e.set_list_fusion(fusion)
        assert e.list_fusion() == int(fusion)
        out.append(e)
    return scene, out[0], out[1]


def _variants(M):
    return 2 if M == 8 else 1  # (the laser hypothesis is member 7)


def _stat_bits(stats):
    return [sorted((k, _bits(float(v)).item()) for k, v in d.items()) for d in stats]


def _hold_state(a, b, n, flags, perturbed, what):
    """what the score left on the two ensembles"""
    for m in range(a.M):
        ma, mb = a.member(m), b.member(m)
        assert _same(ma.costs_view(), mb.costs_view()) and _same(ma.cost_terms(), mb.cost_terms()), (what, m)
        assert _same(ma.knots(0, n), mb.knots(0, n)), (what, m)
        if perturbed and flags & KEEP:
            assert _same(ma.normals(0, n), mb.normals(0, n)), (what, m)
    for mode in ("mean", "max"):
        (ca, ra, ba), (cb, rb, bb) = a.aggregate(mode), b.aggregate(mode)
        assert _same(ca, cb) and np.array_equal(ra, rb) and ba == bb, (what, mode)
    (sa, ua, wa), (sb, ub, wb) = a.blend(L4, want_weights=True), b.blend(L4, want_weights=True)
    assert _stat_bits(sa) == _stat_bits(sb) and _same(ua, ub) and _same(wa, wb), what
    if perturbed:
        (sa, ua, _), (sb, ub, _) = a.blend(L4, gamma=0.7), b.blend(L4, gamma=0.7)
        assert _stat_bits(sa) == _stat_bits(sb) and _same(ua, ub), what


def _hold_scores(scene, a, b, n, flags, launches):
    rs, ga = scene.robot_state, bl.HOLO_GA
    vx, vy, vth = bl._commands(n, 41, 3)
    (ca, ra, ba), (cb, rb, bb) = (e.score_sequences(rs, vx, vth, STEPS, ga, vy=vy, mode="mean") for e in (a, b))
    assert _same(ca, cb) and np.array_equal(ra, rb) and ba == bb
    assert np.any(ca >= 0)
    da, db = a.batch_desc(), b.batch_desc()
    assert da["one_launch_members"] == a.M and da["own_path_members"] == 0 and da["batch_launches"] == launches, da
    assert db["one_launch_members"] == 0 and db["own_path_members"] == b.M and db["batch_launches"] == 0, db
    _hold_state(a, b, n, flags, False, "sequences")
    args = (rs, n, 77, _nominal(3), bl.SIGMA, bl.WIDE[0], bl.WIDE[1], STEPS, ga)
    (ca, ra, ba), (cb, rb, bb) = (e.score_perturbed(*args, flags=flags, mode="max") for e in (a, b))
    assert _same(ca, cb) and np.array_equal(ra, rb) and ba == bb
    assert a.batch_desc()["batch_launches"] == launches
    _hold_state(a, b, n, flags, True, "perturbed")


def _hold_runs(scene, a, b, n, flags, launches, cases):
    rs, ga = scene.robot_state, bl.HOLO_GA
    for gamma, mode, risk in cases:
        for e in (a, b):
            e.set_risk(*risk) if risk else e.clear_risk()
        args = (rs, n, 500 + n, _nominal(3), bl.SIGMA, bl.WIDE[0], bl.WIDE[1], STEPS, ga, ITER, 1.0, gamma)
        ra, rb = (e.mppi_run(*args, flags=flags, mode=mode, want_costs=True) for e in (a, b))
        what = (gamma, mode, risk)
        assert _stat_bits(ra[0]) == _stat_bits(rb[0]) and _same(ra[1], rb[1]) and ra[2] == rb[2], what
        assert _same(ra[3], rb[3]) and np.array_equal(ra[4], rb[4]), what
        assert any(s["n_valid"] > 0 for s in rb[0]), what  # (a condition on the scene: the chain updates the plan)
        da, db = a.batch_desc(), b.batch_desc()
        # one batched launch per variant present in every iteration; the member table goes up in iteration 0 and — its records
        # carrying the arena fetch of the stage only then — at most once more: fewer uploads than iterations
        assert da["one_launch_members"] == a.M and da["batch_launches"] == launches and 1 <= da["table_uploads"] < ITER, da
        assert db["one_launch_members"] == 0 and db["batch_launches"] == 0 and db["table_uploads"] == 0, db
        _hold_state(a, b, n, flags, True, what)
    for e in (a, b):
        e.clear_risk()


@pytest.mark.parametrize("M", [1, 3, 8])
def test_fused_ensemble_is_the_unfused_one(hip_mod, M):
    scene, a, b = _pair(hip_mod, M)
    flags = KEEP if M == 3 else 0
    _hold_scores(scene, a, b, 65, flags, _variants(M))
    _hold_runs(scene, a, b, 65, flags, _variants(M), [(0.0, "mean", None), (0.3, "max", None), (0.3, "mean", (0.5, 0.25))])
    a.close()
    b.close()


def test_sixty_four_members(hip_mod):
    scene, a, b = _pair(hip_mod, 64)
    _hold_scores(scene, a, b, 16, 0, 1)
    _hold_runs(scene, a, b, 16, 0, 1, [(0.3, "mean", None)])
    assert a.batch_desc()["batch_blocks"] == 64 * 16
    a.close()
    b.close()


def test_cycle_fused_off_falls_back_to_the_own_path(hip_mod, monkeypatch):
    scene, a, b = _pair(hip_mod, 3)
    rs, ga = scene.robot_state, bl.HOLO_GA
    args = (rs, 65, 565, _nominal(3), bl.SIGMA, bl.WIDE[0], bl.WIDE[1], STEPS, ga, ITER, 1.0, 0.3)
    want = b.mppi_run(*args, flags=KEEP, want_costs=True)
    monkeypatch.setenv("SFW_CYCLE_FUSED", "0")
    got = a.mppi_run(*args, flags=KEEP, want_costs=True)
    d = a.batch_desc()
    assert d["one_launch_members"] == 0 and d["own_path_members"] == 3 and d["batch_launches"] == 0 and d["table_uploads"] == 0, d
    monkeypatch.delenv("SFW_CYCLE_FUSED")
    assert _stat_bits(got[0]) == _stat_bits(want[0]) and _same(got[1], want[1]) and got[2] == want[2]
    assert _same(got[3], want[3]) and np.array_equal(got[4], want[4])
    _hold_state(a, b, 65, KEEP, True, "unfused")
    a.close()
    b.close()
