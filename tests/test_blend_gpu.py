"""Softmin blend (sfw_grid_blend) on the device, held to include/sfw_hip.h and to the numpy mirror
(social_force_window_planner_amd/blend.py):
  1. weights: the device's exp against numpy's on the same argument (two IEEE operations on the same doubles) — 4 ulp: the
     3 ulp the OpenCL full profile allows a double exp (the accuracy class the device library is written to; no accuracy
     table of ROCm's own is installed beside the library) + glibc's 1 ulp; exact ones, exact zeros;
  2. sums: with the device's own weights handed to blend.reference, eta, sum_w2, every u, j_min, n_valid and index_min are
     bitwise the mirror's — grid, list and sequence stages, with and without bias and vy;
  3. agreement with the launch's selection; 4. independence of how the launch ran and of how the blend was asked;
  5. read-only; 6. bias; 7. refusals, state, no valid sample, batch members; 8. the mean limit.
"Bitwise" compares uint64 views.  The scenes are the synthetic 32-step scenes of tests/test_sequences_gpu.py."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from social_force_window_planner_amd import blend
from social_force_window_planner_amd import synthetic as syn
from social_force_window_planner_amd._abi import (SFW_COST_INVALID, SFW_COST_SKIPPED, SFW_ERR_INVALID_ARG, SFW_ERR_STATE,
                                                   SfwBlendStat)
from sfw_test_util import _bits, _commands, _knot_steps, _params, _same, _scorer, _workload

pytestmark = pytest.mark.gpu

GRAN = 0.03125
HOLO_GA = (1.0, 0.7, 1.0, 2.0, 0.5)
BC = blend.C
SIZES = [1, 63, 64, 65, BC - 1, BC, BC + 1, 2 * BC + 3]
L16 = [float(x) for x in np.geomspace(1e-3, 1e3, 16)]
ULP4 = 2.0 ** -50
# 5 people; 20 people with 16 laser points; 5 people behind a lethal block that rejects the fast straight samples
SCENE_KEYS = [(5, 12, 0), (20, 14, 16), "lethal"]


# ---- the scenes and helpers of tests/test_sequences_gpu.py -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(key):
    """(cached and never written to)"""
    if key == "lethal":  # a lethal block on the x axis 0.3 m ahead, point footprint
        base = syn.make_scene(_workload(5, 12, 0, footprint="point"))
        cells = base.cells.copy()
        my, mx = int((0.0 - base.origin_y) / base.resolution), int((0.3 - base.origin_x) / base.resolution)
        cells[my - 1:my + 1, mx:mx + 2] = 254
        return dataclasses.replace(base, cells=cells)
    if key == "wall":  # every cell lethal: no sample is valid
        base = syn.make_scene(_workload(5, 12, 0))
        return dataclasses.replace(base, cells=np.full_like(base.cells, 254))
    return syn.make_scene(_workload(*key))


# ---- stages -------------------------------------------------------------------------------------------------------------------------
def _knots(vx, vy, vth):
    """(K, n) arrays -> the mirror's (K, 3, n)"""
    return np.stack([vx, np.zeros_like(vx) if vy is None else vy, vth], axis=1)


def _grid_knots(lin, ang):
    vx, vth = np.repeat(lin, len(ang)), np.tile(ang, len(lin))
    return _knots(vx[None, :], None, vth[None, :])


def _score_sequences(g, scene, n, K, seed, holonomic=True):
    """stage + launch + fetch of n random K-knot sequences: (costs, best, knots[K, 3, n])"""
    vx, vy, vth = _commands(n, seed, K, holonomic)
    g.stage_sequences(scene.robot_state, vx, vth, _knot_steps(K), HOLO_GA, vy=vy)
    g.launch()
    costs, best, _ = g.fetch()
    return costs.copy(), best, _knots(vx, vy, vth)


def _stat_key(stats):
    return [(_bits(s["lambda"]).item(), _bits(s["j_min"]).item(), _bits(s["eta"]).item(), _bits(s["sum_w2"]).item(), s["n_valid"],
             s["index_min"]) for s in stats]


def _same_result(a, b, weights=True):
    return (_stat_key(a[0]) == _stat_key(b[0]) and _same(a[1], b[1]) and
            (not weights or (a[2] is None and b[2] is None) or _same(a[2], b[2])))


def _hold_to_mirror(costs, knots, lambdas, bias, got):
    """point 2: the device's sums against the mirror fed with the device's weights, bitwise"""
    stats, u, w = got
    ms, mu, _ = blend.reference(costs, knots, lambdas, bias, weights=w)
    assert _stat_key(stats) == _stat_key(ms), (stats, ms)
    assert _same(u, mu), np.argwhere(_bits(u) != _bits(mu))


def _hold_weights(costs, lambdas, bias, stats, w):
    """point 1: returns the largest relative difference seen, in ulps of 2^-52"""
    valid = costs >= 0
    assert np.all(w[:, ~valid] == 0.0) and not np.any(np.signbit(w))
    worst = 0.0
    if not valid.any():
        return worst
    J = costs + bias if bias is not None else costs
    j_min = stats[0]["j_min"]
    assert j_min == J[valid].min()
    for l, lam in enumerate(lambdas):
        with np.errstate(over="ignore", under="ignore"):
            ref = np.exp(-((J[valid] - j_min) / lam))
        dev = w[l][valid]
        assert np.all(dev[J[valid] == j_min] == 1.0)
        big = ref >= 1e-300
        rel = np.abs(dev[big] - ref[big]) / ref[big]
        assert np.all(rel <= ULP4), (lam, rel.max() / 2.0 ** -52)
        assert np.all(dev[~big] <= 1e-299)
        worst = max(worst, float(rel.max() / 2.0 ** -52))
    return worst


# ---- 1 + 2. weights and sums over the sizes at which a wave or block boundary can go wrong -------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_sequences_weights_and_sums(hip_mod, n):
    key = SCENE_KEYS[SIZES.index(n) % 3]
    scene = _scene(key)
    g = _scorer(hip_mod, scene)
    costs, best, knots = _score_sequences(g, scene, n, 3, 100 + n)
    bias = np.random.default_rng(n).uniform(-2.0, 2.0, n)
    worst = 0.0
    for lambdas in ([0.7], L16):
        for b in (None, bias):
            got = g.blend(lambdas, bias=b, want_weights=True)
            assert got[1].shape == (len(lambdas), 3, 3) and got[2].shape == (len(lambdas), n)
            assert [s["lambda"] for s in got[0]] == list(lambdas)
            assert all(s["n_valid"] == best["n_valid"] == int(np.sum(costs >= 0)) for s in got[0])
            worst = max(worst, _hold_weights(costs, lambdas, b, got[0], got[2]))
            _hold_to_mirror(costs, knots, lambdas, b, got)
    print(f"blend weights n={n} scene={key}: largest |device exp - numpy exp| = {worst:.3f} ulp")
    g.close()


@pytest.mark.parametrize("n,K,L", [(65, 1, 1), (BC + 1, 1, 16), (65, 64, 16), (2 * BC + 3, 64, 1), (BC - 1, 64, 16)])
def test_knot_counts_and_temperature_counts(hip_mod, n, K, L):
    scene = _scene((20, 14, 16))
    g = _scorer(hip_mod, scene)
    lambdas = L16[:L] if L > 1 else [2.5]
    for holonomic in (True, False):
        costs, _, knots = _score_sequences(g, scene, n, K, 7 * n + K, holonomic)
        got = g.blend(lambdas, want_weights=True)
        assert got[1].shape == (L, K, 3)
        if not holonomic:
            assert np.all(got[1][:, :, 1] == 0.0)
        _hold_weights(costs, lambdas, None, got[0], got[2])
        _hold_to_mirror(costs, knots, lambdas, None, got)
    g.close()


@pytest.mark.parametrize("key", SCENE_KEYS)
def test_grid_and_list_stages(hip_mod, key):
    scene = _scene(key)
    g = _scorer(hip_mod, scene)
    lin, ang = syn.reference_sampler()
    costs, best = g.score_grid(scene.robot_state, lin, ang, scene.goal_args)
    skipped = np.flatnonzero(costs == SFW_COST_SKIPPED)
    assert len(skipped) == 1
    bias = np.random.default_rng(3).uniform(-1.0, 1.0, len(costs))
    for b in (None, bias):
        got = g.blend(L16, bias=b, want_weights=True)
        assert np.all(got[2][:, skipped[0]] == 0.0) and np.all(got[1][:, :, 1] == 0.0) and got[1].shape == (16, 1, 3)
        assert all(s["n_valid"] == best["n_valid"] for s in got[0])
        _hold_weights(costs, L16, b, got[0], got[2])
        _hold_to_mirror(costs, _grid_knots(lin, ang), L16, b, got)
    if key == "lethal":
        assert np.any(costs == SFW_COST_INVALID) and np.any(costs >= 0)
    # a grid of more than one block, no (0, 0) sample in it
    lin2, ang2 = syn.generalised_sampler(19, 28)
    costs, best = g.score_grid(scene.robot_state, lin2[1:], ang2, scene.goal_args)
    got = g.blend([0.3, 4.0], want_weights=True)
    _hold_weights(costs, [0.3, 4.0], None, got[0], got[2])
    _hold_to_mirror(costs, _grid_knots(lin2[1:], ang2), [0.3, 4.0], None, got)
    # lists, with and without vy
    for holonomic in (True, False):
        vx, vy, vth = _commands(BC + 1, 21, 1, holonomic)
        costs, best = g.score_samples(scene.robot_state, vx[0], vth[0], HOLO_GA, vy=None if vy is None else vy[0])
        if key == "lethal":
            assert np.any(costs == SFW_COST_INVALID) and np.any(costs >= 0)
        for b in (None, np.linspace(-1.0, 1.0, len(costs))):
            got = g.blend(L16, bias=b, want_weights=True)
            assert all(s["n_valid"] == best["n_valid"] for s in got[0])
            _hold_weights(costs, L16, b, got[0], got[2])
            _hold_to_mirror(costs, _knots(vx, vy, vth), L16, b, got)
    g.close()


def test_coldest_temperature_keeps_the_minimum_only(hip_mod):
    scene = _scene((5, 12, 0))
    g = _scorer(hip_mod, scene)
    costs, best, knots = _score_sequences(g, scene, BC + 1, 3, 55)
    stats, u, w = g.blend([1e-300], want_weights=True)
    valid = costs >= 0
    at_min = valid & (costs == costs[valid].min())
    assert np.all(w[0][at_min] == 1.0) and np.all(w[0][~at_min] == 0.0)
    g.close()


# ---- 3. agreement with the launch ----------------------------------------------------------------------------------------------------
def test_agrees_with_the_selection(hip_mod):
    scene = _scene("lethal")
    g = _scorer(hip_mod, scene)
    n = BC + 1
    vx, vy, vth = _commands(n, 77, 3)
    g.stage_sequences(scene.robot_state, vx, vth, _knot_steps(3), HOLO_GA, vy=vy)
    g.launch()
    costs, best, _ = g.fetch()
    valid = costs >= 0
    assert 0 < valid.sum() < n
    # a duplicate of the cheapest sample behind it: a tie, the larger index holds the minimum
    t0 = int(np.flatnonzero(valid & (costs == costs[valid].min()))[-1])
    t1 = n - 1 if t0 != n - 1 else n - 2
    for a in (vx, vy, vth):
        a[:, t1] = a[:, t0]
    g.stage_sequences(scene.robot_state, vx, vth, _knot_steps(3), HOLO_GA, vy=vy)
    g.launch()
    costs, best, _ = g.fetch()
    valid = costs >= 0
    assert _same(costs[t0], costs[t1])
    stats, u, w = g.blend([0.5, 1e-300], want_weights=True)
    holders = np.flatnonzero(valid & (costs == costs[valid].min()))
    assert len(holders) >= 2
    for s in stats:
        assert s["n_valid"] == best["n_valid"] == int(valid.sum())
        assert s["j_min"] == costs[valid].min() and s["index_min"] == int(holders[-1])
    assert stats[1]["eta"] == float(len(holders))
    # lambda -> 0 with a unique minimum returns that sample's knots
    costs, best, knots = _score_sequences(g, scene, n, 3, 78)
    valid = costs >= 0
    holders = np.flatnonzero(valid & (costs == costs[valid].min()))
    assert len(holders) == 1
    stats, u, _ = g.blend([1e-300])
    assert stats[0]["eta"] == 1.0 and stats[0]["sum_w2"] == 1.0 and _same(u[0], knots[:, :, holders[0]])
    g.close()


# n equal terms x: the butterfly's partial sums are 2x, 4x, ... 64x and a second wave makes 128x — powers of two times x, exact
# for ANY double x —, the rest of the tree adds +0.0, and the division by eta = n is exact too.  So for n = 64 and n = 128 the
# command comes back bit for bit whatever its mantissa holds.  At any other n the sum n * x needs mantissa bits a random
# command does not have to spare (three waves already form 192x = 3 * 64x, one rounding): there the mean is held bitwise
# through the mirror, and the identity itself with commands that have the bits (the next test).
@pytest.mark.parametrize("n", [64, 128, 65, 2 * BC + 3])
def test_identical_samples_return_their_command(hip_mod, n):
    scene = _scene((5, 12, 0))
    g = _scorer(hip_mod, scene)
    vx, vy, vth = _commands(1, 9, 3)
    vx, vy, vth = (np.repeat(a, n, axis=1) for a in (vx, vy, vth))
    g.stage_sequences(scene.robot_state, vx, vth, _knot_steps(3), HOLO_GA, vy=vy)
    g.launch()
    costs, best, _ = g.fetch()
    assert costs[0] >= 0 and np.all(_bits(costs) == _bits(costs[0]))
    lambdas = [1e-300, 1e-3, 1.0, 1e3, 1e300]
    stats, u, w = g.blend(lambdas, want_weights=True)
    assert np.all(w == 1.0)
    for l in range(len(lambdas)):
        assert stats[l]["eta"] == float(n) and stats[l]["sum_w2"] == float(n) and stats[l]["index_min"] == n - 1
        if n in (64, 128):
            assert _same(u[l], _knots(vx, vy, vth)[:, :, 0])
    _hold_to_mirror(costs, _knots(vx, vy, vth), lambdas, None, (stats, u, w))
    g.close()


def test_identical_dyadic_samples_are_returned_bitwise(hip_mod):
    """commands of at most four mantissa bits: every partial sum m * x, m <= n < 2^10, is exact, so at ANY n the mean is the
    command bit for bit"""
    scene = _scene((5, 12, 0))
    g = _scorer(hip_mod, scene)
    n = 2 * BC + 3
    vx = np.repeat(np.array([[0.5], [0.25], [0.625]]), n, axis=1)
    vy = np.repeat(np.array([[0.125], [-0.25], [0.0]]), n, axis=1)
    vth = np.repeat(np.array([[-0.375], [0.5], [0.0625]]), n, axis=1)
    g.stage_sequences(scene.robot_state, vx, vth, _knot_steps(3), HOLO_GA, vy=vy)
    g.launch()
    costs, _, _ = g.fetch()
    assert costs[0] >= 0
    stats, u, _ = g.blend(L16)
    for l in range(16):
        assert stats[l]["eta"] == float(n) and _same(u[l], _knots(vx, vy, vth)[:, :, 0])
    g.close()


# ---- 4. independence -------------------------------------------------------------------------------------------------------------------
def test_independent_of_how_the_launch_ran(hip_mod, monkeypatch):
    scene = _scene((20, 14, 16))
    bias = np.random.default_rng(4).uniform(-1.0, 1.0, 2100)
    g = _scorer(hip_mod, scene)
    # a control cycle's stage: the one-launch kernel and the three-kernel path
    costs, _, knots = _score_sequences(g, scene, 65, 3, 41)
    assert g.plan_info()["one_launch"] == 1
    ref = g.blend(L16, bias=bias[:65], want_weights=True)
    monkeypatch.setenv("SFW_CYCLE_FUSED", "0")
    costs2, _, _ = _score_sequences(g, scene, 65, 3, 41)
    assert g.plan_info()["one_launch"] == 0 and _same(costs, costs2)
    assert _same_result(g.blend(L16, bias=bias[:65], want_weights=True), ref)
    monkeypatch.delenv("SFW_CYCLE_FUSED")
    # 2100 samples in one chunk, chunked, and on a handle that believes in 32 compute units
    costs, _, knots = _score_sequences(g, scene, 2100, 3, 42)
    assert g.plan_info()["chunks"] == 1
    ref = g.blend(L16, bias=bias, want_weights=True)
    _hold_to_mirror(costs, knots, L16, bias, ref)
    # L = 16 against sixteen calls of L = 1; with and without weights_out; twice in a row
    for l in range(16):
        one = g.blend([L16[l]], bias=bias, want_weights=True)
        assert _stat_key(one[0]) == _stat_key(ref[0][l:l + 1]) and _same(one[1][0], ref[1][l]) and _same(one[2][0], ref[2][l]), l
    assert _same_result(g.blend(L16, bias=bias), ref, weights=False)
    assert _same_result(g.blend(L16, bias=bias, want_weights=True), ref)
    monkeypatch.setenv("SFW_TABLE_BUDGET_MB", "1")
    g2 = _scorer(hip_mod, scene)
    costs2, _, _ = _score_sequences(g2, scene, 2100, 3, 42)
    assert g2.plan_info()["chunks"] > 1 and _same(costs, costs2)
    assert _same_result(g2.blend(L16, bias=bias, want_weights=True), ref)
    monkeypatch.delenv("SFW_TABLE_BUDGET_MB")
    monkeypatch.setenv("SFW_DEVICE_CUS", "32")
    g3 = _scorer(hip_mod, scene)
    monkeypatch.delenv("SFW_DEVICE_CUS")
    costs3, _, _ = _score_sequences(g3, scene, 2100, 3, 42)
    assert _same(costs, costs3)
    assert _same_result(g3.blend(L16, bias=bias, want_weights=True), ref)
    for h in (g, g2, g3):
        h.close()


# ---- 5. read-only ------------------------------------------------------------------------------------------------------------------------
def test_read_only_for_the_launch(hip_mod):
    scene = _scene((20, 14, 16))
    g = _scorer(hip_mod, scene)
    g.set_terms_capture(True)
    g.set_points_capture(True)
    weights = [[1.0, 2.0, 0.5, 1.0, 3.0], [0.0, 1.0, 0.0, 0.0, 1.0]]
    for n in (65, 2 * BC + 3):
        costs, best, knots = _score_sequences(g, scene, n, 3, 60 + n)
        view = g.costs_view().copy()
        pts = g.grid_points(best["index"])
        terms = g.cost_terms()
        rb, rc = g.rescore(weights, want_costs=True)
        crowd = g.grid_crowd(best["index"])
        g.blend(L16, bias=np.linspace(-3.0, 3.0, n), want_weights=True)
        g.blend([0.1])
        assert _same(g.costs_view(), view) and _same(view, costs)
        c2, b2, _ = g.fetch()
        assert _same(c2, costs) and b2 == best
        assert _same(g.grid_points(best["index"]), pts) and _same(g.cost_terms(), terms)
        rb2, rc2 = g.rescore(weights, want_costs=True)
        assert rb2 == rb and _same(rc2, rc)
        crowd2 = g.grid_crowd(best["index"])
        assert _same(crowd2["state"], crowd["state"]) and _same(crowd2["work"], crowd["work"]) and _same(crowd2["cost"], crowd["cost"])
        # ... and the blend still answers after them
        _hold_to_mirror(costs, knots, [0.1], None, g.blend([0.1], want_weights=True))
    g.close()


# ---- 6. bias ---------------------------------------------------------------------------------------------------------------------------
def test_bias(hip_mod):
    scene = _scene("lethal")
    g = _scorer(hip_mod, scene)
    n = BC + 1
    costs, best, knots = _score_sequences(g, scene, n, 3, 81)
    valid = costs >= 0
    assert 0 < valid.sum() < n
    ref = g.blend(L16, want_weights=True)
    # an all-zero bias is the NULL bias
    assert _same_result(g.blend(L16, bias=np.zeros(n), want_weights=True), ref)
    # bias at invalid samples changes nothing
    junk = np.where(valid, 0.0, np.random.default_rng(1).uniform(-1e6, 1e6, n))
    assert _same_result(g.blend(L16, bias=junk, want_weights=True), ref)
    # a valid sample that is not the minimum becomes it
    j_min = ref[0][0]["j_min"]
    t = int(np.flatnonzero(valid & (costs > j_min))[0])
    bias = np.zeros(n)
    bias[t] = -((costs[t] - j_min) + 0.25)
    stats, u, w = g.blend(L16, bias=bias, want_weights=True)
    assert all(s["index_min"] == t and s["j_min"] == costs[t] + bias[t] for s in stats)
    assert np.all(w[:, t] == 1.0)
    _hold_weights(costs, L16, bias, stats, w)
    _hold_to_mirror(costs, knots, L16, bias, (stats, u, w))
    g.close()


# ---- 7. refusals and state --------------------------------------------------------------------------------------------------------------
def _raw_blend(hip_mod, g, lam, L, bias, stat, u, w=None):
    lam_p = None if lam is None else np.ascontiguousarray(lam, dtype=np.float64).ctypes.data
    bias_a = None if bias is None else np.ascontiguousarray(bias, dtype=np.float64)
    return hip_mod.lib().sfw_grid_blend(g._h, lam_p, L, None if bias_a is None else bias_a.ctypes.data, stat,
                                        None if u is None else u.ctypes.data, None if w is None else w.ctypes.data)


def test_refusals_change_nothing(hip_mod):
    scene = _scene((5, 12, 0))
    g = _scorer(hip_mod, scene)
    n = 65
    costs, best, knots = _score_sequences(g, scene, n, 3, 90)
    ref = g.blend(L16, want_weights=True)
    stat, u = (SfwBlendStat * 16)(), np.zeros((16, 3, 3))
    nan_bias, inf_bias = np.zeros(n), np.zeros(n)
    nan_bias[n - 1], inf_bias[0] = np.nan, np.inf
    refused = [
        (None, 1, None, stat, u), ([1.0], 1, None, None, u), ([1.0], 1, None, stat, None),
        ([1.0], 0, None, stat, u), ([1.0], -3, None, stat, u), ([1.0] * 17, 17, None, stat, u),
        ([0.0], 1, None, stat, u), ([-1.0], 1, None, stat, u), ([1.0, np.nan], 2, None, stat, u), ([np.inf], 1, None, stat, u),
        ([1.0], 1, nan_bias, stat, u), ([1.0], 1, inf_bias, stat, u),
    ]
    for args in refused:
        assert _raw_blend(hip_mod, g, *args) == SFW_ERR_INVALID_ARG, args[:2]
        assert _same_result(g.blend(L16, want_weights=True), ref)
    assert hip_mod.lib().sfw_grid_blend(None, None, 1, None, None, None, None) == SFW_ERR_INVALID_ARG
    c2, b2, _ = g.fetch()
    assert _same(c2, costs) and b2 == best
    g.close()


def test_state_machine(hip_mod):
    scene = _scene((5, 12, 0))
    g = _scorer(hip_mod, scene)
    stat, u = (SfwBlendStat * 1)(), np.zeros((1, 64, 3))
    assert _raw_blend(hip_mod, g, [1.0], 1, None, stat, u) == SFW_ERR_STATE  # nothing staged, nothing launched
    with pytest.raises(hip_mod.SfwError) as e:
        g.blend([1.0])
    assert e.value.status == SFW_ERR_STATE
    vx, vy, vth = _commands(65, 91, 3)
    g.stage_sequences(scene.robot_state, vx, vth, _knot_steps(3), HOLO_GA, vy=vy)
    assert _raw_blend(hip_mod, g, [1.0], 1, None, stat, u) == SFW_ERR_STATE  # staged, not launched
    g.launch()
    assert _raw_blend(hip_mod, g, [1.0], 1, None, stat, u) == 0  # before any fetch: the call waits for the launch itself
    costs, _, _ = g.fetch()
    _hold_to_mirror(costs, _knots(vx, vy, vth), [1.0], None, g.blend([1.0], want_weights=True))
    g.stage_sequences(scene.robot_state, vx, vth, _knot_steps(3), HOLO_GA, vy=vy)  # a new stage without a launch
    assert _raw_blend(hip_mod, g, [1.0], 1, None, stat, u) == SFW_ERR_STATE
    g.launch()
    g.fetch()
    assert _raw_blend(hip_mod, g, [1.0], 1, None, stat, u) == 0
    g.score_one(scene.robot_state, 0.3, 0.0, 0.1, scene.goal_args)
    assert _raw_blend(hip_mod, g, [1.0], 1, None, stat, u) == SFW_ERR_STATE
    with pytest.raises(hip_mod.SfwError) as e:
        g.blend([1.0])
    assert e.value.status == SFW_ERR_STATE
    g.close()


@pytest.mark.parametrize("n", [45, BC + 1])
def test_no_valid_sample(hip_mod, n):
    scene = _scene("wall")
    g = _scorer(hip_mod, scene)
    costs, best, knots = _score_sequences(g, scene, n, 3, 92)
    assert np.all(costs == SFW_COST_INVALID) and best["n_valid"] == 0
    stats, u, w = g.blend(L16, bias=np.ones(n), want_weights=True)
    for l in range(16):
        assert stats[l] == {"lambda": L16[l], "j_min": -1.0, "eta": 0.0, "sum_w2": 0.0, "n_valid": 0, "index_min": -1, "ess": 0.0}
    assert np.all(_bits(u) == 0) and np.all(_bits(w) == 0)
    _hold_to_mirror(costs, knots, L16, None, (stats, u, w))
    g.close()


def test_batch_members(hip_mod):
    scene = _scene((5, 12, 0))
    lin, ang = syn.reference_sampler()
    lx, ly, lth = _commands(20, 37)
    vx, vy, vth = _commands(30, 38, K=3)
    steps = _knot_steps(3)
    rs, ga = scene.robot_state, scene.goal_args
    alone = _scorer(hip_mod, scene)
    want = []
    alone.score_sequences(rs, vx, vth, steps, HOLO_GA, vy=vy)
    want.append(alone.blend(L16, want_weights=True))
    alone.score_samples(rs, lx[0], lth[0], HOLO_GA, vy=ly[0])
    want.append(alone.blend(L16, want_weights=True))
    alone.score_grid(rs, lin, ang, ga)
    want.append(alone.blend(L16, want_weights=True))
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
        got = bs.member(i).blend(L16, want_weights=True)
        assert got[1].shape == want[i][1].shape and _same_result(got, want[i]), i
        assert got[0][0]["n_valid"] == bests[i]["n_valid"]
    bs.close()


# ---- 8. the mean limit ------------------------------------------------------------------------------------------------------------------
def test_hottest_temperature_is_the_plain_mean(hip_mod):
    scene = _scene("lethal")
    g = _scorer(hip_mod, scene)
    n = 2 * BC + 3
    costs, best, knots = _score_sequences(g, scene, n, 3, 95)
    valid = costs >= 0
    assert 0 < valid.sum() < n
    stats, u, w = g.blend([1e300], want_weights=True)
    assert np.all(w[0][~valid] == 0.0) and np.all(np.abs(w[0][valid] - 1.0) <= 2.0 ** -52)
    _hold_to_mirror(costs, knots, [1e300], None, (stats, u, w))
    # the plain mean over the valid samples, through the same tree
    ones = valid.astype(np.float64)[None, :]
    ms, mu, _ = blend.reference(costs, knots, [1e300], weights=ones)
    if np.all(w[0][valid] == 1.0):
        assert _same(u, mu) and stats[0]["eta"] == float(valid.sum()) == ms[0]["eta"]
    g.close()
