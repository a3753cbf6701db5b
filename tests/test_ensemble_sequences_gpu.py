"""sfw_ensemble_score_sequences / _score_perturbed / _blend: MPPI rollouts under several crowd hypotheses.

Scenes and hypotheses are those of tests/test_ensemble_gpu.py: the reference's scene (5 people: the members take the one-launch
cycle) and the 8-person cfg2 variant (they do not), under its six mixed hypotheses.  Commands come from a seeded generator as in
tests/test_sequences_gpu.py, holonomic and not, over a box wide enough (|vx| <= 3 m/s under 6 m/s^2) that within the 1 s horizon
some samples reach a person of some crowds only, and some a person of every crowd.  On the CPU oracle — which scores one
command per sample: the K = 1 lists, and of a K > 1 case the samples `_commands` keeps constant — every case of n >= 63 holds
valid samples, samples rejected by 1 .. M - 1 hypotheses and samples rejected by all M, in both scenes, with the seeds of
`SEED_SHIFT`; the perturbed draws are aimed at the edge of the commands every hypothesis rejects (`NOMINAL_AT`).  Every test
asserts all three kinds (`_hold_mix`) in every case but n = 1, where one sample is one kind; copies of one hypothesis reject
together, so there the middle kind cannot exist.
Sample counts are the edges of a wave and of one and two 256-sample blocks (the selection's block and the blend's).
"Bitwise" compares uint64 views."""
import ctypes as C
import dataclasses
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from social_force_window_planner_amd import blend, perturb
from social_force_window_planner_amd import synthetic as syn
from social_force_window_planner_amd._abi import (SFW_COST_INVALID, SFW_COST_SKIPPED, SFW_ERR_INVALID_ARG, SFW_ERR_STATE, SFW_OK,
                                                   SFW_PERTURB_KEEP_NOMINAL, SFW_PERTURB_KEEP_NORMALS, SFW_PERTURB_NO_VY,
                                                   SFW_PRECISION_F32, SFW_PRECISION_F64, SFW_PRECISION_F64_STRICT, SfwAgent,
                                                   SfwBest, SfwBlendStat, SfwGoalArgs, SfwRobotState)
from social_force_window_planner_amd.hypotheses import naive_goal_hypotheses
from test_blend_gpu import ULP4  # the bound that file holds the device exp to
from sfw_test_util import _bits, _np_best, _same, _scene_params as _params

pytestmark = pytest.mark.gpu

WEIGHT_FIELDS = ("vel_weight", "distance_weight", "angle_weight", "costmap_weight", "social_weight")
SCENES = ("ref5x9", "cfg2_8")
HOLO_GA = (6.0, 3.0, 6.0, 2.0, 0.5)
NONH_GA = (6.0, 0.0, 6.0, 2.0, 0.5)
V_MAX, VY_MAX, W_MAX = 3.0, 0.5, 1.0
L16 = [float(x) for x in np.geomspace(1e-3, 1e3, 16)]
# (n, K): the sample counts with one and three knots, and the most knots at one sample past a wave
CASES = [(n, K) for n in (1, 63, 257, 513) for K in (1, 3)] + [(65, 64)]
KEEP, NO_VY, NOMINAL = SFW_PERTURB_KEEP_NORMALS, SFW_PERTURB_NO_VY, SFW_PERTURB_KEEP_NOMINAL


# ---- scenes, hypotheses and the definition, as tests/test_ensemble_gpu.py has them ------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(name):
    """(cached and never written to)"""
    if name == "ref5x9":
        return syn.make_scene("ref5x9")
    return syn.make_scene(dataclasses.replace(syn.WORKLOADS["cfg2"], nv=48, nw=48, n_people=8))


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
    return costs, rejected


def _weights(p):
    return tuple(getattr(p, f) for f in WEIGHT_FIELDS)


def _ensemble(hip_mod, scene, hypotheses, params=None):
    e = hip_mod.EnsembleScorer(params if params is not None else _params(scene), 0, len(hypotheses))
    e.load_scene(scene, hypotheses)
    return e


def _standalone(hip_mod, scene, agents, obstacles, params=None):
    g = hip_mod.HipScorer(params if params is not None else _params(scene))
    g.load_scene(scene)
    g.set_agents(agents, obstacles)
    return g


# ---- commands --------------------------------------------------------------------------------------------------------------------
def _commands(n, seed, K=1, holonomic=True):
    """(K, n) arrays of random commands (tests/test_sequences_gpu.py's generator over this file's box).  Every second sample
    keeps its first command over the whole horizon: such a sequence is the K = 1 sample (tests/test_sequences_gpu.py point 2),
    which the CPU oracle can score — that is how the mix of a K > 1 case was checked there."""
    rng = np.random.default_rng(seed)
    vx, vth = rng.uniform(-V_MAX, V_MAX, (K, n)), rng.uniform(-W_MAX, W_MAX, (K, n))
    vy = rng.uniform(-VY_MAX, VY_MAX, (K, n)) if holonomic else None
    for a in (vx, vy, vth):
        if a is not None:
            a[:, ::2] = a[0, ::2]
    return vx, vy, vth


def _knot_steps(K):
    """(40 steps: the last knots of K = 64 lie past the horizon and are ignored)"""
    return tuple(range(K)) if K > 3 else (0, 9, 23)[:K]


# Seeds are family + 10 n + K + 100000 s.  s is 0 unless listed here: the first s at which the samples the CPU oracle can score
# hold at least two of each kind (valid, rejected by some, rejected by all) in both scenes, under the mixed hypotheses and,
# without the middle kind, under the scene's own crowd alone.  From n = 257 on s = 0 does.
SEED_SHIFT = {(63, 1, 5000): 3, (63, 1, 7000): 9, (63, 3, 5000): 2, (63, 3, 7000): 1, (65, 64, 5000): 26, (65, 64, 7000): 19}


def _case(n, K, family=5000):
    """The sequences of a case: holonomic for K = 3, not for K = 1 and K = 64.  (vx, vy, vth, steps, goal args)"""
    holonomic = K == 3
    vx, vy, vth = _commands(n, family + 10 * n + K + 100000 * SEED_SHIFT.get((n, K, family), 0), K, holonomic)
    return vx, vy, vth, _knot_steps(K), HOLO_GA if holonomic else NONH_GA


def _knots(vx, vy, vth):
    """(K, n) arrays -> the blend mirror's (K, 3, n)"""
    return np.stack([vx, np.zeros_like(vx) if vy is None else vy, vth], axis=1)


def _score(e, scene, case, **kw):
    vx, vy, vth, steps, ga = case
    return e.score_sequences(scene.robot_state, vx, vth, steps, ga, vy=vy, **kw)


def _score_handle(g, scene, case):
    vx, vy, vth, steps, ga = case
    return g.score_sequences(scene.robot_state, vx, vth, steps, ga, vy=vy)


def _hold_mix(rejected, M, n, what="", copies=False):
    """The preconditions of a test over n samples (see the module's text): a vacuous run fails here.  copies: the members are
    copies of one hypothesis, which reject together — no sample is rejected by some of them only."""
    valid, partial, by_all = int(np.sum(rejected == 0)), int(np.sum((rejected > 0) & (rejected < M))), int(np.sum(rejected == M))
    print(f"{what} n={n}: {valid} valid, {partial} rejected by some, {by_all} rejected by all of {M}")
    assert valid + partial + by_all == n
    if n > 1:
        assert valid > 0 and by_all > 0 and (partial > 0 or copies), (valid, partial, by_all)


# ---- the blend's checks, as tests/test_blend_gpu.py has them --------------------------------------------------------------------------
def _stat_key(stats):
    return [(_bits(s["lambda"]).item(), _bits(s["j_min"]).item(), _bits(s["eta"]).item(), _bits(s["sum_w2"]).item(), s["n_valid"],
             s["index_min"]) for s in stats]


def _same_result(a, b, weights=True):
    return (_stat_key(a[0]) == _stat_key(b[0]) and _same(a[1], b[1]) and
            (not weights or (a[2] is None and b[2] is None) or _same(a[2], b[2])))


def _hold_to_mirror(costs, knots, lambdas, bias, got):
    """the device's sums against the mirror fed with the device's weights, bitwise"""
    stats, u, w = got
    ms, mu, _ = blend.reference(costs, knots, lambdas, bias, weights=w)
    assert _stat_key(stats) == _stat_key(ms), (stats, ms)
    assert _same(u, mu), np.argwhere(_bits(u) != _bits(mu))


def _hold_weights(costs, lambdas, bias, stats, w):
    """0.0 exactly where c < 0, 1.0 exactly at j_min, the device exp within ULP4 elsewhere"""
    valid = costs >= 0
    assert np.all(w[:, ~valid] == 0.0) and not np.any(np.signbit(w))
    if not valid.any():
        return
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


def _blends(n):
    """(lambdas, bias) of L = 1 and L = 16, with and without bias"""
    bias = np.random.default_rng(n).uniform(-2.0, 2.0, n)
    return [([0.7], None), ([0.7], bias), (L16, None), (L16, bias)]


# ---- 1. M = 1, MEAN with p = {1}: the standalone handle -----------------------------------------------------------------------------
def _check_is_the_handle(hip_mod, scene, n, K, precision, M, mode, probs):
    p = _params(scene, precision)
    e = _ensemble(hip_mod, scene, [(scene.agents, scene.obstacles)] * M, p)
    g = _standalone(hip_mod, scene, scene.agents, scene.obstacles, p)
    case = _case(n, K)
    costs, rejected, best = _score(e, scene, case, mode=mode, probs=probs)
    gc, gb = _score_handle(g, scene, case)
    assert _same(costs, gc), f"{int(np.sum(_bits(costs) != _bits(gc)))} costs differ"
    assert best == gb
    assert not np.any(costs == SFW_COST_SKIPPED) and not np.any(np.isnan(costs))
    assert np.array_equal(rejected, M * (gc == SFW_COST_INVALID).astype(np.int32))
    _hold_mix(rejected, M, n, "copies" if M > 1 else "single", copies=True)
    for m in range(M):
        assert _same(e.member(m).costs_view(), gc)
    for lambdas, bias in _blends(n):
        got, want = e.blend(lambdas, bias=bias, want_weights=True), g.blend(lambdas, bias=bias, want_weights=True)
        assert got[1].shape == (len(lambdas), K, 3) and got[2].shape == (len(lambdas), n)
        assert _same_result(got, want), (len(lambdas), bias is not None)
    e.close()
    g.close()


@pytest.mark.parametrize("scene_name", SCENES)
@pytest.mark.parametrize("n,K", CASES)
def test_single_member_is_the_handle(hip_mod, scene_name, n, K):
    _check_is_the_handle(hip_mod, _scene(scene_name), n, K, SFW_PRECISION_F64, 1, "mean", [1.0])


@pytest.mark.parametrize("scene_name", SCENES)
@pytest.mark.parametrize("precision", [SFW_PRECISION_F32, SFW_PRECISION_F64_STRICT])
def test_single_member_in_other_precisions(hip_mod, scene_name, precision):
    _check_is_the_handle(hip_mod, _scene(scene_name), 257, 3, precision, 1, "mean", [1.0])


# ---- 2. M copies under MAX ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene_name", SCENES)
@pytest.mark.parametrize("n,K", [(1, 3), (63, 1), (257, 3), (513, 1), (65, 64)])
def test_copies_under_max_are_the_handle(hip_mod, scene_name, n, K):
    _check_is_the_handle(hip_mod, _scene(scene_name), n, K, SFW_PRECISION_F64, 4, "max", None)


# ---- 3. mixed hypotheses against the definition -------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene_name", SCENES)
@pytest.mark.parametrize("n,K", CASES)
def test_mixed_hypotheses_match_the_definition(hip_mod, scene_name, n, K):
    scene = _scene(scene_name)
    hyps = _mixed_hypotheses(scene)
    M = len(hyps)
    p = _params(scene)
    e = _ensemble(hip_mod, scene, hyps, p)
    case = _case(n, K)
    vx, vy, vth = case[:3]
    for mode, probs in (("mean", None), ("mean", [0.5, 0.1, 0.1, 0.1, 0.15, 0.3]), ("max", None)):
        costs, rejected, best = _score(e, scene, case, mode=mode, probs=probs)
        terms = [e.member(m).cost_terms() for m in range(M)]
        assert all(t.shape == (n, 5) for t in terms)
        hc, hr = _host_ensemble(terms, _weights(p), mode, probs)
        assert np.array_equal(rejected, hr)
        assert _same(costs, hc), f"{mode}: {int(np.sum(_bits(costs) != _bits(hc)))} costs differ"
        assert not np.any(costs == SFW_COST_SKIPPED)
        assert best == _np_best(hc, vx[0], None if vy is None else vy[0], vth[0])
        assert best["n_valid"] == int(np.sum(rejected == 0))
        if best["index"] >= 0:
            t = best["index"]
            assert _same([best["vx"], best["vy"], best["vtheta"]], [vx[0, t], 0.0 if vy is None else vy[0, t], vth[0, t]])
        # the re-aggregation is the score
        ac, ar, ab = e.aggregate(mode, probs)
        assert _same(ac, costs) and np.array_equal(ar, rejected) and ab == best
    _hold_mix(rejected, M, n, "mixed")
    print("one_launch by member:", [e.member(m).plan_info()["one_launch"] for m in range(M)])
    # every member against a standalone handle with its hypothesis; its knots are the sequences
    g = _standalone(hip_mod, scene, scene.agents, scene.obstacles, p)
    for m, (agents, obs) in enumerate(hyps):
        g.set_agents(agents, obs)
        gc, _ = _score_handle(g, scene, case)
        assert _same(e.member(m).costs_view(), gc), f"member {m}"
        assert _same(e.member(m).knots(0, n), _knots(vx, vy, vth)), f"member {m}"
    assert _same(e.knots(0, n), _knots(vx, vy, vth))
    g.close()
    e.close()


# ---- 4. perturbed -------------------------------------------------------------------------------------------------------------------
WIDE = ((-V_MAX, -VY_MAX, -W_MAX), (V_MAX, VY_MAX, W_MAX))
SIGMA = (1.0, 0.25, 0.35)
# The nominal plan of a scene's perturbed cases heads for the edge of the commands that every hypothesis rejects (on the CPU
# oracle: vx >= 1.5 turning right in the reference's scene, vx <= -2.5 turning right in the cfg2 variant), so that draws of
# SIGMA around it fall on both sides of it and into the commands that reach the added person only.
NOMINAL_AT = {"ref5x9": (2.0, 0.0, -0.6), "cfg2_8": (-2.6, 0.0, -0.7)}


def _nominal(K, no_vy=False, at=(0.5, 0.0, -0.05)):
    k = np.arange(K, dtype=np.float64)
    nom = np.stack([at[0] + 0.1 * np.cos(k), at[1] + 0.05 * np.sin(k), at[2] + 0.05 * np.sin(0.7 * k)], axis=1)
    if no_vy:
        nom[:, 1] = 0.0
    return nom


def _perturbed_steps(K):
    """Three knots inside the 40-step horizon, the others past it (drawn, read back and blended, ignored by the rollout): noise
    redrawn at every step of the horizon averages out, and all 65 samples of the K = 64 case would be of the nominal plan's kind
    (measured: no valid sample in the cfg2 variant with a knot per step)"""
    return _knot_steps(K) if K <= 3 else (0, 9, 23) + tuple(range(40, 40 + K - 3))


def _perturbed_case(scene_name, n, K, flags):
    """(seed, nominal, sigma, knot steps, goal args) of a perturbed case"""
    no_vy = bool(flags & NO_VY)
    return (900 + n + K, _nominal(K, no_vy, NOMINAL_AT[scene_name]), (SIGMA[0], 0.0, SIGMA[2]) if no_vy else SIGMA, _perturbed_steps(K),
            NONH_GA if no_vy else HOLO_GA)


@pytest.mark.parametrize("scene_name", SCENES)
@pytest.mark.parametrize("n,K,flags", [(1, 3, 0), (63, 1, NOMINAL), (257, 3, NO_VY), (513, 3, NOMINAL | NO_VY), (513, 1, 0),
                                       (65, 64, NOMINAL)])
def test_perturbed_scoring(hip_mod, scene_name, n, K, flags):
    scene = _scene(scene_name)
    hyps = _mixed_hypotheses(scene)
    M = len(hyps)
    e = _ensemble(hip_mod, scene, hyps)
    no_vy = bool(flags & NO_VY)
    seed, nominal, sigma, steps, ga = _perturbed_case(scene_name, n, K, flags)
    for mode in ("mean", "max"):
        costs, rejected, best = e.score_perturbed(scene.robot_state, n, seed, nominal, sigma, WIDE[0], WIDE[1], steps, ga,
                                                  flags=flags | KEEP, mode=mode)
        # every member drew the knots of the definition (the mirror, fed with the device's own normals), bitwise the same M times
        u = e.member(0).knots(0, n)
        z = e.member(0).normals(0, n)
        assert u.shape == (K, 3, n)
        assert _same(u, perturb.reference(seed, nominal, sigma, WIDE[0], WIDE[1], n, flags=flags, normals=z))
        if flags & NOMINAL:
            assert _same(u[:, :, 0], nominal)
        if no_vy:
            assert np.all(_bits(u[:, 1, :]) == 0)
        for m in range(1, M):
            assert _same(e.member(m).knots(0, n), u), f"member {m}"
        assert _same(e.knots(0, n), u)
        # the winner's command is its first knot as the device holds it
        if best["index"] >= 0:
            assert _same([best["vx"], best["vy"], best["vtheta"]], e.knots(best["index"], 1)[0, :, 0])
        else:
            assert (best["vx"], best["vy"], best["vtheta"]) == (0.0, 0.0, 0.0)
        # the results are those of the same knots handed over by the host
        sc, sr, sb = e.score_sequences(scene.robot_state, u[:, 0, :], u[:, 2, :], steps, ga, vy=None if no_vy else u[:, 1, :], mode=mode)
        assert _same(costs, sc) and np.array_equal(rejected, sr) and best == sb
    _hold_mix(rejected, M, n, "perturbed")
    e.close()


# ---- 5. the blend over the ensemble costs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene_name", SCENES)
@pytest.mark.parametrize("n,K", CASES)
def test_blend_over_the_ensemble_costs(hip_mod, scene_name, n, K):
    scene = _scene(scene_name)
    hyps = _mixed_hypotheses(scene)
    M = len(hyps)
    e = _ensemble(hip_mod, scene, hyps)
    case = _case(n, K, family=7000)
    knots = _knots(*case[:3])
    costs, rejected, best = _score(e, scene, case, mode="mean")
    _hold_mix(rejected, M, n, "blend")
    first = {}
    for i, (lambdas, bias) in enumerate(_blends(n)):
        got = e.blend(lambdas, bias=bias, want_weights=True)
        assert got[1].shape == (len(lambdas), K, 3) and got[2].shape == (len(lambdas), n)
        assert all(s["n_valid"] == best["n_valid"] for s in got[0])
        _hold_weights(costs, lambdas, bias, got[0], got[2])
        _hold_to_mirror(costs, knots, lambdas, bias, got)
        assert _same_result(e.blend(lambdas, bias=bias), got, weights=False)  # (without weights_out; repeated)
        first[i] = got
    # after a re-aggregation the blend reads ITS costs; back under MEAN it is bitwise what it was
    mc, mr, mb = e.aggregate("max")
    lambdas, bias = _blends(n)[3]
    got = e.blend(lambdas, bias=bias, want_weights=True)
    assert all(s["n_valid"] == mb["n_valid"] for s in got[0])
    _hold_weights(mc, lambdas, bias, got[0], got[2])
    _hold_to_mirror(mc, knots, lambdas, bias, got)
    if np.any((costs >= 0) & (_bits(mc) != _bits(costs))) and n > 1:
        assert not _same(got[2], first[3][2]), "the blend did not follow the re-aggregation"
    ac, _, _ = e.aggregate("mean")
    assert _same(ac, costs)
    assert _same_result(e.blend(lambdas, bias=bias, want_weights=True), first[3])
    e.close()


def _grid_knots(lin, ang):
    vx, vth = np.repeat(lin, len(ang)), np.tile(ang, len(lin))
    return _knots(vx[None, :], None, vth[None, :])


@pytest.mark.parametrize("scene_name", SCENES)
def test_blend_after_a_grid_score(hip_mod, scene_name):
    scene = _scene(scene_name)
    e = _ensemble(hip_mod, scene, _mixed_hypotheses(scene))
    costs, rejected, best = e.score_grid(scene.robot_state, scene.linvels, scene.angvels, scene.goal_args, mode="mean")
    T = len(costs)
    assert np.any(costs >= 0)
    for lambdas, bias in _blends(T):
        got = e.blend(lambdas, bias=bias, want_weights=True)
        assert got[1].shape == (len(lambdas), 1, 3) and np.all(got[1][:, :, 1] == 0.0)
        assert all(s["n_valid"] == best["n_valid"] for s in got[0])
        _hold_weights(costs, lambdas, bias, got[0], got[2])
        _hold_to_mirror(costs, _grid_knots(scene.linvels, scene.angvels), lambdas, bias, got)
    mc, _, mb = e.aggregate("max")
    got = e.blend(L16, want_weights=True)
    _hold_to_mirror(mc, _grid_knots(scene.linvels, scene.angvels), L16, None, got)
    e.close()


@pytest.mark.parametrize("n", [45, 257])
def test_blend_without_a_valid_sample(hip_mod, n):
    """one person standing on the robot (10 cm off its centre) in ONE hypothesis rejects every sample of the ensemble"""
    scene = _scene("ref5x9")
    hyps = _mixed_hypotheses(scene)[:3]
    hyps[1] = (_with_person(scene.agents, 0.1, 0.0, 0.0, 0.0), scene.obstacles)
    e = _ensemble(hip_mod, scene, hyps)
    case = _case(n, 3)
    costs, rejected, best = _score(e, scene, case, mode="mean")
    assert np.all(costs == SFW_COST_INVALID) and np.all(rejected >= 1) and np.any(rejected < 3)
    assert best["n_valid"] == 0 and best["index"] == -1
    stats, u, w = e.blend(L16, bias=np.ones(n), want_weights=True)
    for l in range(16):
        assert stats[l] == {"lambda": L16[l], "j_min": -1.0, "eta": 0.0, "sum_w2": 0.0, "n_valid": 0, "index_min": -1, "ess": 0.0}
    assert np.all(_bits(u) == 0) and np.all(_bits(w) == 0)
    e.close()


# ---- 6. independence of how the launch ran and of where the costs went ---------------------------------------------------------------
def _everything(e, scene, case, n):
    """(score, MAX re-aggregation, the blend of both) of one ensemble"""
    out = [_score(e, scene, case, mode="mean")]
    bias = np.random.default_rng(n + 1).uniform(-1.0, 1.0, n)
    out.append(e.blend(L16, bias=bias, want_weights=True))
    out.append(e.aggregate("max"))
    out.append(e.blend(L16, bias=bias, want_weights=True))
    return out


def _same_everything(a, b):
    for (ca, ra, ba), (cb, rb, bb) in ((a[0], b[0]), (a[2], b[2])):
        if not (_same(ca, cb) and np.array_equal(ra, rb) and ba == bb):
            return False
    return _same_result(a[1], b[1]) and _same_result(a[3], b[3])


@pytest.mark.parametrize("scene_name", SCENES)
def test_independent_of_how_the_launch_ran(hip_mod, monkeypatch, scene_name):
    scene = _scene(scene_name)
    hyps = _mixed_hypotheses(scene)
    for n in (63, 2100):
        case = _case(n, 3)
        e = _ensemble(hip_mod, scene, hyps)
        ref = _everything(e, scene, case, n)
        _hold_mix(ref[0][1], len(hyps), n, "independence")
        assert e.member(0).plan_info()["chunks"] == 1
        # the cost vector past the pinned mirror's limit: the aggregation leaves it on the device and copies it out
        monkeypatch.setenv("SFW_MIRROR_MAX_MB", "0")
        e2 = _ensemble(hip_mod, scene, hyps)
        monkeypatch.delenv("SFW_MIRROR_MAX_MB")
        got = _everything(e2, scene, case, n)
        assert e2.member(0).costs_view() is None  # (the members' launches were not mirrored either)
        assert _same_everything(got, ref), "mirror limit"
        e2.close()
        # without the one-launch cycle
        monkeypatch.setenv("SFW_CYCLE_FUSED", "0")
        got = _everything(e, scene, case, n)
        assert e.member(0).plan_info()["one_launch"] == 0
        monkeypatch.delenv("SFW_CYCLE_FUSED")
        assert _same_everything(got, ref), "SFW_CYCLE_FUSED=0"
        # chunked launches
        if n == 2100:
            monkeypatch.setenv("SFW_TABLE_BUDGET_MB", "1")
            e3 = _ensemble(hip_mod, scene, hyps)
            monkeypatch.delenv("SFW_TABLE_BUDGET_MB")
            got = _everything(e3, scene, case, n)
            assert e3.member(0).plan_info()["chunks"] > 1
            assert _same_everything(got, ref), "chunked"
            e3.close()
        e.close()


# ---- 7. state and refusals ----------------------------------------------------------------------------------------------------------
def _ptr(a):
    return None if a is None else a.ctypes.data


def _raw_sequences(hip_mod, e, rs, vx, vy, vth, n, K, steps, ga, mode=0, probs=None):
    steps_a = None if steps is None else np.ascontiguousarray(steps, dtype=np.int32)
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (vx, vy, vth, probs)]
    costs, rej, best = np.zeros(max(n, 1)), np.zeros(max(n, 1), dtype=np.int32), SfwBest()
    return hip_mod.lib().sfw_ensemble_score_sequences(
        e._e, None if rs is None else C.byref(SfwRobotState(*rs)), _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]), n, K, _ptr(steps_a),
        None if ga is None else C.byref(SfwGoalArgs(*ga)), mode, _ptr(arrs[3]), costs.ctypes.data, rej.ctypes.data, C.byref(best))


def _raw_perturbed(hip_mod, e, rs, p, n, K, steps, ga, mode=0):
    steps_a = None if steps is None else np.ascontiguousarray(steps, dtype=np.int32)
    costs, rej, best = np.zeros(max(n, 1)), np.zeros(max(n, 1), dtype=np.int32), SfwBest()
    return hip_mod.lib().sfw_ensemble_score_perturbed(
        e._e, None if rs is None else C.byref(SfwRobotState(*rs)), None if p is None else C.byref(p), n, K, _ptr(steps_a),
        None if ga is None else C.byref(SfwGoalArgs(*ga)), mode, None, costs.ctypes.data, rej.ctypes.data, C.byref(best))


def _raw_blend(hip_mod, e, lam, L, bias, stat, u):
    lam_a = None if lam is None else np.ascontiguousarray(lam, dtype=np.float64)
    bias_a = None if bias is None else np.ascontiguousarray(bias, dtype=np.float64)
    return hip_mod.lib().sfw_ensemble_blend(e._e, _ptr(lam_a), L, _ptr(bias_a), stat, _ptr(u), None)


def test_refusals_leave_the_previous_score_usable(hip_mod):
    scene = _scene("ref5x9")
    hyps = _mixed_hypotheses(scene)
    e = _ensemble(hip_mod, scene, hyps)
    n, K = 65, 3
    case = _case(n, K)
    vx, vy, vth, steps, ga = case
    rs = scene.robot_state
    ref_score = _score(e, scene, case, mode="mean")
    ref_blend = e.blend(L16, want_weights=True)

    def unchanged(what):
        c, r, b = e.aggregate("mean")
        assert _same(c, ref_score[0]) and np.array_equal(r, ref_score[1]) and b == ref_score[2], what
        assert _same_result(e.blend(L16, want_weights=True), ref_blend), what

    bad = vx.copy()
    bad[2, n - 1] = np.nan
    bad_vy = vy.copy()
    bad_vy[0, 0] = np.inf
    good = dict(rs=rs, vx=vx, vy=vy, vth=vth, n=n, K=K, steps=steps, ga=ga)
    refused = [dict(mode=7), dict(probs=[0.5, -0.1, 0.2, 0.2, 0.1, 0.1]), dict(probs=[np.nan] * 6),
               dict(K=0), dict(K=65), dict(steps=None), dict(steps=(1, 9, 23)), dict(steps=(0, 9, 9)), dict(steps=(0, 23, 9)),
               dict(rs=None), dict(vx=None), dict(vth=None), dict(ga=None), dict(n=0), dict(n=-4),
               dict(vx=bad), dict(vth=bad), dict(vy=bad_vy), dict(rs=(0.0, np.nan, 0.0, 0.3, 0.0, 0.0)),
               dict(ga=(6.0, 3.0, np.inf, 2.0, 0.5))]
    for change in refused:
        assert _raw_sequences(hip_mod, e, **{**good, **change}) == SFW_ERR_INVALID_ARG, list(change)
        unchanged(list(change))
    nominal = _nominal(K)
    zero_vy = nominal.copy()
    zero_vy[:, 1] = 0.0

    def perturb_of(nominal=nominal, sigma=SIGMA, lo=WIDE[0], hi=WIDE[1], flags=0, reserved=0, null_nominal=False):
        p, nom, _ = hip_mod.HipScorer._perturb(3, nominal, sigma, lo, hi, steps, flags)
        p.reserved = reserved
        if null_nominal:
            p.nominal = None
        return p, nom

    nan_nominal = nominal.copy()
    nan_nominal[1, 2] = np.nan
    refused = [dict(p=None), dict(p=perturb_of(null_nominal=True)), dict(rs=None), dict(ga=None), dict(steps=None), dict(n=0),
               dict(K=0), dict(K=65), dict(steps=(2, 9, 23)), dict(steps=(0, 9, 9)), dict(p=perturb_of(flags=8)),
               dict(p=perturb_of(reserved=1)), dict(p=perturb_of(nominal=nan_nominal)), dict(p=perturb_of(sigma=(0.1, -0.1, 0.1))),
               dict(p=perturb_of(lo=(0.0, 0.0, 0.6), hi=(0.7, 0.3, 0.5))), dict(p=perturb_of(flags=NO_VY)),
               dict(p=perturb_of(sigma=(1.5, 0.0, 0.5), flags=NO_VY)), dict(mode=2)]
    ok_p = perturb_of(nominal=zero_vy, sigma=(1.5, 0.0, 0.5), flags=NO_VY)  # (the pair keeps the nominal array alive)
    assert _raw_perturbed(hip_mod, e, rs, ok_p[0], n, K, steps, NONH_GA) == SFW_OK
    _score(e, scene, case, mode="mean")
    unchanged("a fresh score")
    good = dict(rs=rs, p=perturb_of(), n=n, K=K, steps=steps, ga=ga)
    for change in refused:
        args = {**good, **change}
        if isinstance(args["p"], tuple):
            args["p"] = args["p"][0]
        assert _raw_perturbed(hip_mod, e, **args) == SFW_ERR_INVALID_ARG, list(change)
        unchanged(list(change))
    stat, u = (SfwBlendStat * 16)(), np.zeros((16, K, 3))
    nan_bias = np.zeros(n)
    nan_bias[n - 1] = np.nan
    for lam, L, bias, st, uu in [(None, 1, None, stat, u), ([1.0], 1, None, None, u), ([1.0], 1, None, stat, None),
                                 ([1.0], 0, None, stat, u), ([1.0] * 17, 17, None, stat, u), ([0.0], 1, None, stat, u),
                                 ([1.0, np.nan], 2, None, stat, u), ([np.inf], 1, None, stat, u), ([1.0], 1, nan_bias, stat, u)]:
        assert _raw_blend(hip_mod, e, lam, L, bias, st, uu) == SFW_ERR_INVALID_ARG, (lam, L)
        unchanged((lam, L))
    # the accepted call still runs
    assert _raw_perturbed(hip_mod, e, **{**good, "p": good["p"][0]}) == SFW_OK
    e.close()


def test_state_rules(hip_mod):
    scene = _scene("ref5x9")
    hyps = _mixed_hypotheses(scene)[:3]
    rs = scene.robot_state
    case = _case(65, 3)
    # a hypothesis never set
    e = hip_mod.EnsembleScorer(_params(scene), 0, 3)
    e.set_costmap(scene.cells, scene.origin_x, scene.origin_y, scene.resolution)
    e.set_footprint(scene.footprint)
    e.set_hypothesis(0, *hyps[0])
    e.set_hypothesis(2, *hyps[2])
    for call in (lambda: _score(e, scene, case),
                 lambda: e.score_perturbed(rs, 65, 1, _nominal(3), SIGMA, WIDE[0], WIDE[1], _knot_steps(3), HOLO_GA)):
        with pytest.raises(hip_mod.SfwError) as ex:
            call()
        assert ex.value.status == SFW_ERR_STATE and "hypothesis 1" in str(ex.value)
    # nothing scored
    for call in (lambda: e.blend([1.0]), lambda: e.aggregate("mean")):
        with pytest.raises(hip_mod.SfwError) as ex:
            call()
        assert ex.value.status == SFW_ERR_STATE
    e.set_hypothesis(1, *hyps[1])
    costs, rejected, best = _score(e, scene, case)
    ref_blend = e.blend(L16, want_weights=True)
    assert best["index"] >= 0
    # a member's own calls after the ensemble's blend return what they returned before it
    m0 = e.member(0)
    own_blend, own_crowd = m0.blend(L16, want_weights=True), m0.grid_crowd(best["index"])
    assert _same_result(e.blend(L16, want_weights=True), ref_blend)
    again = m0.grid_crowd(best["index"])
    assert _same_result(m0.blend(L16, want_weights=True), own_blend)
    assert _same(again["cost"], own_crowd["cost"]) and _same(again["state"], own_crowd["state"]) and _same(again["work"], own_crowd["work"])
    assert _same(m0.costs_view(), m0.fetch()[0])
    assert _same_result(e.blend(L16, want_weights=True), ref_blend)  # (reading a member is no new stage)
    # a member staged since / used for sfw_score_one since
    vx, vy, vth, steps, ga = case
    e.member(1).stage_sequences(rs, vx, vth, steps, ga, vy=vy)
    for call in (lambda: e.blend([1.0]), lambda: e.aggregate("mean")):
        with pytest.raises(hip_mod.SfwError) as ex:
            call()
        assert ex.value.status == SFW_ERR_STATE and "member 1" in str(ex.value)
    _score(e, scene, case)
    assert _same_result(e.blend(L16, want_weights=True), ref_blend)
    e.member(2).score_one(rs, 0.3, 0.0, 0.1, scene.goal_args)
    for call in (lambda: e.blend([1.0]), lambda: e.aggregate("max")):
        with pytest.raises(hip_mod.SfwError) as ex:
            call()
        assert ex.value.status == SFW_ERR_STATE and "member 2" in str(ex.value)
    # parameters changed through a member
    e.member(1).set_params(_params(scene, social_weight=2.0))
    with pytest.raises(hip_mod.SfwError) as ex:
        _score(e, scene, case)
    assert ex.value.status == SFW_ERR_STATE
    e.set_params(_params(scene))
    # a grid after sequences and the reverse: the output lengths follow the last score
    c, r, _ = _score(e, scene, case)
    assert len(c) == len(r) == 65 and len(e.aggregate("max")[0]) == 65 and e.blend([1.0])[1].shape == (1, 3, 3)
    gc, gr, gb = e.score_grid(rs, scene.linvels, scene.angvels, scene.goal_args)
    T = len(scene.linvels) * len(scene.angvels)
    ac, ar, ab = e.aggregate("mean")
    assert len(gc) == len(ac) == len(ar) == T and _same(ac, gc) and ab == gb
    stats, u, w = e.blend([1.0], want_weights=True)
    assert u.shape == (1, 1, 3) and w.shape == (1, T)
    c2, r2, b2 = _score(e, scene, _case(63, 1))
    ac, ar, ab = e.aggregate("mean")
    assert len(c2) == len(ac) == 63 and _same(ac, c2) and np.array_equal(ar, r2) and ab == b2
    assert e.blend([1.0], want_weights=True)[2].shape == (1, 63)
    us = e.last_us()
    assert us["stage"] > 0 and us["enqueue"] > 0 and us["wait_fetch"] > 0
    e.close()


# ---- 8. lifetime --------------------------------------------------------------------------------------------------------------------
def test_lifetime(hip_mod):
    scene = _scene("ref5x9")
    hyps = _mixed_hypotheses(scene)
    case = _case(257, 3)
    first = None
    for _ in range(10):
        e = _ensemble(hip_mod, scene, hyps)
        score = _score(e, scene, case, mode="max")
        got = (score, e.blend(L16, want_weights=True))
        e.close()
        if first is None:
            first = got
    assert first[0][2]["n_valid"] > 0
    assert _same(got[0][0], first[0][0]) and np.array_equal(got[0][1], first[0][1]) and got[0][2] == first[0][2]
    assert _same_result(got[1], first[1])
