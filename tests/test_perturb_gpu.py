"""Perturbed sequences (sfw_sequences_perturb_stage) on the device, held to include/sfw_hip.h and to the numpy mirror
(social_force_window_planner_amd/perturb.py):
  1. bits: with the device's own normals handed to perturb.reference the device's knots are bitwise the mirror's;
  2. normals: |z_dev - z_numpy| <= 16 * 2^-53 * r with r = numpy's sqrt(-2 log u1).  Derived, not measured, on the convention
     of tests/test_blend_gpu.py (the device library written to the OpenCL full profile, glibc within 1 ulp): log 3 + 1 ulp
     relative, halved by the root; cos 4 + 1 ulp of a value <= 1; the root's and the product's own roundings: below 12, with a
     margin to 16;
  3. the counter's carry; 4. placement: a value depends on (seed, g, k, c) alone; 5. equivalence: a second handle staged by
  sfw_sequences_stage with the fetched knots is bit for bit the perturbed stage in everything it produces; 6. the winner's
  first knot; 7. refusals; 8. state; 9. repetition; 10. batch members; 11. plan_info and the conservative rest flag.
"Bitwise" compares uint64 views.  The scenes are the synthetic 32-step scenes of tests/test_blend_gpu.py."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from social_force_window_planner_amd import perturb
from social_force_window_planner_amd import synthetic as syn
from social_force_window_planner_amd._abi import (SFW_COST_INVALID, SFW_ERR_INVALID_ARG, SFW_ERR_STATE, SFW_PERTURB_KEEP_NOMINAL,
                                                   SFW_PERTURB_KEEP_NORMALS, SFW_PERTURB_NO_VY, SfwAgent, SfwPerturb)
from sfw_test_util import _bits, _knot_steps, _nominal, _params, _same, _scorer, _workload

pytestmark = pytest.mark.gpu

GRAN = 0.03125
STEPS = 32
HOLO_GA = (1.0, 0.7, 1.0, 2.0, 0.5)
SIZES = [1, 63, 64, 65, 255, 256, 257, 515]
L16 = [float(x) for x in np.geomspace(1e-3, 1e3, 16)]
KEEP, NO_VY, NOMINAL = SFW_PERTURB_KEEP_NORMALS, SFW_PERTURB_NO_VY, SFW_PERTURB_KEEP_NOMINAL
SIGMA = (0.2, 0.1, 0.3)
WIDE = ((0.0, -0.3, -0.5), (0.7, 0.3, 0.5))         # the robot's limits
HALF = ((0.27, -0.04, -0.2), (0.5, 0.07, 0.15))    # cuts about half the draws around _nominal's rows


# ---- the scenes and helpers of tests/test_blend_gpu.py -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(key):
    """(cached and never written to)"""
    if key == "lethal":  # a lethal block on the x axis 0.3 m ahead, point footprint
        base = syn.make_scene(_workload(5, 12, 0, footprint="point"))
        cells = base.cells.copy()
        my, mx = int((0.0 - base.origin_y) / base.resolution), int((0.3 - base.origin_x) / base.resolution)
        cells[my - 1:my + 1, mx:mx + 2] = 254
        return dataclasses.replace(base, cells=cells)
    if key == "pinned":  # (5, 12, 0) with person 1 pinned: desired_velocity 0, standing 1.2 m ahead to the left
        base = syn.make_scene(_workload(5, 12, 0))
        agents = (SfwAgent * len(base.agents))()
        for a in range(len(base.agents)):
            C.memmove(C.byref(agents[a]), C.byref(base.agents[a]), C.sizeof(SfwAgent))
        p = agents[1]
        p.x, p.y, p.vx, p.vy, p.has_goal, p.desired_velocity = 1.2, 0.4, 0.0, 0.0, 0, 0.0
        return dataclasses.replace(base, agents=agents)
    return syn.make_scene(_workload(*key))


def _stage(g, scene, n, K, seed, flags=0, box=WIDE, sigma=SIGMA, index_base=0, nominal=None):
    no_vy = bool(flags & NO_VY)
    nominal = _nominal(K, no_vy) if nominal is None else nominal
    sigma = (sigma[0], 0.0, sigma[2]) if no_vy else sigma
    g.stage_perturbed(scene.robot_state, n, seed, nominal, sigma, box[0], box[1], _knot_steps(K), HOLO_GA, flags=flags,
                      index_base=index_base)
    return nominal, sigma


def _hold_normals(z, seed, n, K, index_base=0, flags=0):
    """point 2: returns the largest |z_dev - z_numpy| seen, in multiples of 2^-53 * r"""
    ref = perturb.normals(seed, n, K, index_base, flags)
    u1, _ = perturb.uniforms(seed, n, K, index_base)
    r = perturb.radius(seed, n, K, index_base)
    assert z.shape == ref.shape == (K, 3, n)
    assert np.all(np.abs(z) < 8.58)
    assert np.all(z[u1 == 1.0] == 0.0) and np.all(ref[u1 == 1.0] == 0.0)
    if flags & NOMINAL and index_base == 0:
        assert np.all(_bits(z[:, :, 0]) == 0)
    err = np.abs(z - ref)
    bound = 16.0 * 2.0 ** -53 * r
    assert np.all(err <= bound), float(np.max(err[r > 0] / (2.0 ** -53 * r[r > 0])))
    return float(np.max(err[r > 0] / (2.0 ** -53 * r[r > 0]))) if np.any(r > 0) else 0.0


# ---- 1 + 2. bits and normals over the sizes at which a wave or block boundary can go wrong ------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_knots_are_the_mirror_of_the_device_normals(hip_mod, n):
    scene = _scene((5, 12, 0))
    g = _scorer(hip_mod, scene)
    worst, cut = 0.0, []
    for K in (1, 3, 64):
        for flags in (0, NO_VY, NOMINAL, NO_VY | NOMINAL):
            for box in (WIDE, HALF):
                seed = 1000 * n + 10 * K + flags
                nominal, sigma = _stage(g, scene, n, K, seed, flags | KEEP, box)
                z, u = g.normals(0, n), g.knots(0, n)
                assert z.shape == u.shape == (K, 3, n)
                want = perturb.reference(seed, nominal, sigma, box[0], box[1], n, flags=flags, normals=z)
                assert _same(u, want), (K, flags, np.argwhere(_bits(u) != _bits(want))[:4])
                worst = max(worst, _hold_normals(z, seed, n, K, flags=flags))
                if flags & NO_VY:
                    assert np.all(_bits(u[:, 1, :]) == 0)
                if flags & NOMINAL and box is WIDE:
                    assert _same(u[:, :, 0], nominal)
                if box is HALF:
                    raw = nominal[:, :, None] + np.asarray(sigma)[None, :, None] * z
                    ch = [0, 2] if flags & NO_VY else [0, 1, 2]
                    lo, hi = np.asarray(box[0])[None, ch, None], np.asarray(box[1])[None, ch, None]
                    cut.append(((raw[:, ch] < lo) | (raw[:, ch] > hi)).mean())
                # a sub-range reads back what the whole range holds
                first, count = n // 3, max(1, n // 2)
                assert _same(g.knots(first, count), u[:, :, first:first + count])
                assert _same(g.normals(first, count), z[:, :, first:first + count])
    if n >= 255:
        assert 0.3 < float(np.mean(cut)) < 0.7, np.mean(cut)
    print(f"perturb normals n={n}: largest |device z - numpy z| = {worst:.3f} x 2^-53 r")
    g.close()


# ---- 3. the counter's carry -----------------------------------------------------------------------------------------------------------
def test_counter_carries_into_its_second_word(hip_mod):
    scene = _scene((5, 12, 0))
    g = _scorer(hip_mod, scene)
    base, n, K, seed = 2 ** 32 - 3, 8, 3, (0x9E3779B9 << 32) | 0x7F4A7C15
    nominal, sigma = _stage(g, scene, n, K, seed, KEEP | NOMINAL, index_base=base)
    z, u = g.normals(0, n), g.knots(0, n)
    worst = _hold_normals(z, seed, n, K, index_base=base, flags=NOMINAL)
    assert _same(u, perturb.reference(seed, nominal, sigma, WIDE[0], WIDE[1], n, index_base=base, flags=NOMINAL, normals=z))
    assert len(np.unique(z)) == z.size and not np.any(z[:, :, 0] == 0.0)  # (global sample 0 is not in this shard)
    print(f"perturb carry: largest |device z - numpy z| = {worst:.3f} x 2^-53 r")
    g.launch()
    _, best, key = g.fetch()
    assert key[3] == -(base + best["index"])
    g.close()


# ---- 4. placement ---------------------------------------------------------------------------------------------------------------------
def _draw(g, scene, n, K, seed, **kw):
    _stage(g, scene, n, K, seed, KEEP, **kw)
    return g.knots(0, n), g.normals(0, n)


def test_a_value_depends_on_seed_sample_knot_and_channel_alone(hip_mod, monkeypatch):
    scene = _scene((20, 14, 16))
    g = _scorer(hip_mod, scene)
    u, z = _draw(g, scene, 130, 3, 77)
    ua, za = _draw(g, scene, 65, 3, 77)
    ub, zb = _draw(g, scene, 65, 3, 77, index_base=65)
    assert _same(u[:, :, :65], ua) and _same(u[:, :, 65:], ub) and _same(z[:, :, :65], za) and _same(z[:, :, 65:], zb)
    u515, z515 = _draw(g, scene, 515, 3, 78)
    u64, z64 = _draw(g, scene, 64, 3, 78)
    assert _same(u515[:, :, :64], u64) and _same(z515[:, :, :64], z64)
    nom64 = _nominal(64)
    u_k64, z_k64 = _draw(g, scene, 257, 64, 79, nominal=nom64)
    g.stage_perturbed(scene.robot_state, 257, 79, nom64[:3], SIGMA, WIDE[0], WIDE[1], (0, 1, 2), HOLO_GA, flags=KEEP)
    assert _same(u_k64[:3], g.knots(0, 257)) and _same(z_k64[:3], g.normals(0, 257))
    # the one-launch kernel or the three-kernel path, one chunk or several, 256 or 32 compute units: the same knots and costs
    def scored(h, n, seed):
        _stage(h, scene, n, 3, seed)
        h.launch()
        costs, best, _ = h.fetch()
        return costs.copy(), best, h.knots(0, n), h.plan_info()

    c65, b65, k65, plan = scored(g, 65, 80)
    assert plan["one_launch"] == 1
    monkeypatch.setenv("SFW_CYCLE_FUSED", "0")
    c2, b2, k2, plan = scored(g, 65, 80)
    assert plan["one_launch"] == 0 and _same(c65, c2) and b65 == b2 and _same(k65, k2)
    monkeypatch.delenv("SFW_CYCLE_FUSED")
    c, b, k, plan = scored(g, 2100, 81)
    assert plan["chunks"] == 1
    monkeypatch.setenv("SFW_TABLE_BUDGET_MB", "1")
    g2 = _scorer(hip_mod, scene)
    monkeypatch.delenv("SFW_TABLE_BUDGET_MB")
    c2, b2, k2, plan = scored(g2, 2100, 81)
    assert plan["chunks"] > 1 and _same(c, c2) and b == b2 and _same(k, k2)
    monkeypatch.setenv("SFW_DEVICE_CUS", "32")
    g3 = _scorer(hip_mod, scene)
    monkeypatch.delenv("SFW_DEVICE_CUS")
    c3, b3, k3, _ = scored(g3, 2100, 81)
    assert _same(c, c3) and b == b3 and _same(k, k3)
    for h in (g, g2, g3):
        h.close()


# ---- 5 + 6. equivalence with sfw_sequences_stage over the fetched knots, and the winner ---------------------------------------------
@pytest.mark.parametrize("n,K,key,flags", [(45, 1, (5, 12, 0), 0), (45, 4, "lethal", NO_VY), (257, 1, "lethal", 0),
                                           (257, 4, (20, 14, 16), NOMINAL), (1500, 1, (20, 14, 16), NO_VY | NOMINAL),
                                           (1500, 4, "lethal", 0)])
def test_second_stage_with_the_fetched_knots_is_the_perturbed_stage(hip_mod, n, K, key, flags):
    scene = _scene(key)
    a, b = _scorer(hip_mod, scene), _scorer(hip_mod, scene)
    for h in (a, b):
        h.set_terms_capture(True)
    _stage(a, scene, n, K, 5000 + n + K, flags)
    if n == 45:
        assert a.plan_info()["one_launch"] == 1
    knots = a.knots(0, n)
    b.stage_sequences(scene.robot_state, knots[:, 0], knots[:, 2], _knot_steps(K), HOLO_GA, vy=None if flags & NO_VY else knots[:, 1])
    assert _same(b.knots(0, n), knots)  # (the read-back serves host-staged sequences too)
    pa, pb = a.plan_info(), b.plan_info()
    assert {k: v for k, v in pa.items() if k != "rest_noise_unreproduced"} == {k: v for k, v in pb.items() if k != "rest_noise_unreproduced"}
    got = []
    for h in (a, b):
        h.launch()
        costs, best, sel_key = h.fetch()
        weights = [[1.0, 2.0, 0.5, 1.0, 3.0], [0.0, 1.0, 0.0, 0.0, 1.0]]
        got.append({"costs": costs.copy(), "best": best, "key": sel_key, "terms": h.cost_terms(), "points": h.grid_points_batch(0, n, STEPS),
                    "crowd": h.grid_crowd(best["index"]), "blend1": h.blend([0.7], want_weights=True),
                    "blend16": h.blend(L16, want_weights=True), "rescore": h.rescore(weights, want_costs=True)})
    p, s = got
    assert _same(p["costs"], s["costs"]), np.flatnonzero(_bits(p["costs"]) != _bits(s["costs"]))[:8]
    assert p["best"] == s["best"] and p["key"] == s["key"] and p["best"]["n_valid"] == int(np.sum(p["costs"] >= 0))
    for f in ("cost", "vx", "vy", "vtheta"):
        assert _same(p["best"][f], s["best"][f]), f
    if key == "lethal":
        assert np.any(p["costs"] == SFW_COST_INVALID) and np.any(p["costs"] >= 0)
    assert not np.any(np.isnan(p["costs"])) and np.all((p["costs"] >= 0) | (p["costs"] == SFW_COST_INVALID))
    assert _same(p["terms"], s["terms"])
    assert _same(p["points"][0], s["points"][0]) and np.array_equal(p["points"][1], s["points"][1])
    for f in ("state", "work", "cost"):
        assert _same(p["crowd"][f], s["crowd"][f]), f
    assert np.array_equal(p["crowd"]["has_goal"], s["crowd"]["has_goal"]) and p["crowd"]["n_steps"] == s["crowd"]["n_steps"]
    for name in ("blend1", "blend16"):
        (st_p, u_p, w_p), (st_s, u_s, w_s) = p[name], s[name]
        assert [sorted((k, _bits(float(v)).item()) for k, v in d.items()) for d in st_p] == \
            [sorted((k, _bits(float(v)).item()) for k, v in d.items()) for d in st_s], name
        assert _same(u_p, u_s) and _same(w_p, w_s), name
    assert p["rescore"][0] == s["rescore"][0] and _same(p["rescore"][1], s["rescore"][1])
    # the winner's command is its first knot, bit for bit
    if p["best"]["index"] >= 0:
        first = a.knots(p["best"]["index"], 1)[0, :, 0]
        assert _same([p["best"]["vx"], p["best"]["vy"], p["best"]["vtheta"]], first)
        assert _same(first, knots[0, :, p["best"]["index"]])
    # the blocking call is stage + launch + fetch
    nominal = _nominal(K, bool(flags & NO_VY))
    sigma = (SIGMA[0], 0.0, SIGMA[2]) if flags & NO_VY else SIGMA
    c3, b3 = a.score_perturbed(scene.robot_state, n, 5000 + n + K, nominal, sigma, WIDE[0], WIDE[1], _knot_steps(K), HOLO_GA, flags=flags)
    assert _same(c3, p["costs"]) and b3 == p["best"]
    a.close()
    b.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_staged_grid_alone(hip_mod):
    scene = _scene((5, 12, 0))
    g = _scorer(hip_mod, scene)
    lin, ang = syn.reference_sampler()
    costs, best = g.score_grid(scene.robot_state, lin, ang, scene.goal_args)
    g.stage(scene.robot_state, lin, ang, scene.goal_args)
    L = hip_mod.lib()
    rs, ga = hip_mod.SfwRobotState(*scene.robot_state), hip_mod.SfwGoalArgs(*HOLO_GA)
    ks, many = np.array([0, 7, 19], dtype=np.int32), np.arange(65, dtype=np.int32)
    nom, wide = np.ascontiguousarray(_nominal(3)), np.zeros((65, 3))
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

    def call(p=None, rs_p=C.byref(rs), n=6, K=3, ks_p=ks.ctypes.data, ga_p=C.byref(ga), base=0, null_p=False):
        p = perturb_of() if p is None else p
        return L.sfw_sequences_perturb_stage(g._h, rs_p, None if null_p else C.byref(p), n, K, ks_p, ga_p, base)

    def knots(*v):
        a = np.array(v, dtype=np.int32)
        keep.append(a)
        return a.ctypes.data

    def with_bad(value, at):
        b = nom.copy()
        b[at] = value
        return b

    flat = nom.copy()
    flat[:, 1] = 0.0
    bad_rs = hip_mod.SfwRobotState(0.0, np.nan, 0.0, 0.3, 0.0, 0.0)
    bad_ga = hip_mod.SfwGoalArgs(1.0, 0.7, np.inf, 2.0, 0.5)
    refused = [
        L.sfw_sequences_perturb_stage(None, C.byref(rs), C.byref(perturb_of()), 6, 3, ks.ctypes.data, C.byref(ga), 0),
        call(rs_p=None), call(null_p=True), call(perturb_of(null_nominal=True)), call(ks_p=None), call(ga_p=None),
        call(n=0), call(n=-3), call(K=0), call(K=-1), call(perturb_of(nominal=wide), K=65, ks_p=many.ctypes.data),
        call(ks_p=knots(1, 7, 19)), call(ks_p=knots(0, 7, 7)), call(ks_p=knots(0, 19, 7)),
        call(base=-1),
        call(perturb_of(nominal=with_bad(np.nan, (1, 0)))), call(perturb_of(nominal=with_bad(np.inf, (2, 2)))),
        call(perturb_of(sigma=(0.1, np.nan, 0.1))), call(perturb_of(sigma=(np.inf, 0.1, 0.1))),
        call(perturb_of(lo=(-np.inf, -0.3, -0.5))), call(perturb_of(hi=(0.7, 0.3, np.nan))),
        call(rs_p=C.byref(bad_rs)), call(ga_p=C.byref(bad_ga)),
        call(perturb_of(sigma=(0.1, -0.1, 0.1))), call(perturb_of(sigma=(0.1, 0.1, -1e-300))),
        call(perturb_of(lo=(0.8, -0.3, -0.5))), call(perturb_of(lo=(0.0, -0.3, 0.6))),
        call(perturb_of(flags=8)), call(perturb_of(flags=-1)), call(perturb_of(flags=1 << 30)), call(perturb_of(reserved=1)),
        call(perturb_of(nominal=flat, flags=NO_VY)),                                  # sigma[1] != 0
        call(perturb_of(nominal=nom, sigma=(0.1, 0.0, 0.1), flags=NO_VY)),            # a nominal vy != 0
    ]
    assert refused == [SFW_ERR_INVALID_ARG] * len(refused), refused
    # the read-backs refuse before they touch anything too (a grid is staged: SFW_ERR_STATE whatever the range)
    out = np.zeros(3 * 6 * 3)
    assert L.sfw_sequences_knots(g._h, 0, 6, out.ctypes.data, None, out.ctypes.data) == SFW_ERR_STATE
    assert L.sfw_sequences_normals(g._h, 0, 6, out.ctypes.data) == SFW_ERR_STATE
    g.launch()  # the grid is still staged
    c2, b2, _ = g.fetch()
    assert _same(c2, costs) and b2 == best
    # ... and the limits themselves are accepted
    assert call(perturb_of(nominal=wide, sigma=(0.0, 0.0, 0.0), lo=(0.0, 0.0, 0.0), hi=(0.0, 0.0, 0.0)), K=64, ks_p=many.ctypes.data) == 0
    assert call(perturb_of(nominal=flat, sigma=(0.1, 0.0, 0.1), flags=NO_VY | NOMINAL | KEEP), base=2 ** 40) == 0
    bad_ranges = [(-1, 2), (0, 0), (0, 7), (6, 1), (5, 2), (0, -1)]
    for first, count in bad_ranges:
        assert L.sfw_sequences_knots(g._h, first, count, out.ctypes.data, out.ctypes.data, out.ctypes.data) == SFW_ERR_INVALID_ARG
        assert L.sfw_sequences_normals(g._h, first, count, out.ctypes.data) == SFW_ERR_INVALID_ARG
    assert L.sfw_sequences_knots(g._h, 0, 6, None, None, out.ctypes.data) == SFW_ERR_INVALID_ARG
    assert L.sfw_sequences_knots(g._h, 0, 6, out.ctypes.data, None, None) == SFW_ERR_INVALID_ARG
    assert L.sfw_sequences_normals(g._h, 0, 6, None) == SFW_ERR_INVALID_ARG
    assert L.sfw_sequences_knots(g._h, 5, 1, out.ctypes.data, None, out.ctypes.data) == 0
    g.close()
    # no costmap
    e = hip_mod.HipScorer(_params())
    with pytest.raises(hip_mod.SfwError) as err:
        e.stage_perturbed((0, 0, 0, 0, 0, 0), 4, 1, _nominal(2), SIGMA, WIDE[0], WIDE[1], (0, 5), HOLO_GA)
    assert err.value.status == SFW_ERR_STATE
    e.close()


# ---- 8 + 9. state and repetition ------------------------------------------------------------------------------------------------------
def test_state_machine_and_repetition(hip_mod):
    scene = _scene((5, 12, 0))
    rs = scene.robot_state
    g = _scorer(hip_mod, scene)
    with pytest.raises(hip_mod.SfwError) as e:  # nothing staged
        g.knots(0, 1)
    assert e.value.status == SFW_ERR_STATE
    _stage(g, scene, 30, 3, 11)  # without KEEP_NORMALS
    with pytest.raises(hip_mod.SfwError) as e:
        g.normals(0, 30)
    assert e.value.status == SFW_ERR_STATE
    first = g.knots(0, 30)
    # the same seed draws the same bits, another seed other bits; keeping the normals changes no knot
    _stage(g, scene, 30, 3, 11, KEEP)
    assert _same(g.knots(0, 30), first)
    z = g.normals(0, 30)
    _stage(g, scene, 30, 3, 12, KEEP)
    assert np.mean(g.knots(0, 30) == first) < 0.2 and not np.any(g.normals(0, 30) == z)  # (equal only where both are clamped)
    _stage(g, scene, 30, 3, 11 + (1 << 32), KEEP)  # the seed's high word is key material too
    assert not np.any(g.normals(0, 30) == z)
    # grid, list, sequences and perturbed stages replace one another
    lin, ang = syn.reference_sampler()
    lx, lth = np.linspace(0.1, 0.6, 20), np.linspace(-0.4, 0.4, 20)
    vx, vth = np.tile(lx, (3, 1)), np.tile(lth, (3, 1)) * np.array([[1.0], [0.5], [-1.0]])
    gc, gb = g.score_grid(rs, lin, ang, scene.goal_args)
    lc, lb = g.score_samples(rs, lx, lth, HOLO_GA)
    sc, sb = g.score_sequences(rs, vx, vth, (0, 7, 19), HOLO_GA)
    nominal = _nominal(3)
    pc, pb = g.score_perturbed(rs, 30, 11, nominal, SIGMA, WIDE[0], WIDE[1], (0, 7, 19), HOLO_GA)
    stage = {"grid": lambda: g.stage(rs, lin, ang, scene.goal_args), "list": lambda: g.stage_samples(rs, lx, lth, HOLO_GA),
             "seq": lambda: g.stage_sequences(rs, vx, vth, (0, 7, 19), HOLO_GA), "perturbed": lambda: _stage(g, scene, 30, 3, 11)}
    want = {"grid": (gc, gb, 45), "list": (lc, lb, 20), "seq": (sc, sb, 20), "perturbed": (pc, pb, 30)}
    for a, b in (("grid", "perturbed"), ("perturbed", "grid"), ("list", "perturbed"), ("perturbed", "list"), ("seq", "perturbed"),
                 ("perturbed", "seq"), ("perturbed", "perturbed")):
        stage[a]()
        stage[b]()
        assert g.plan_info()["samples"] == want[b][2]
        g.launch()
        c, best, _ = g.fetch()
        assert _same(c, want[b][0]) and best == want[b][1], (a, b)
        if b == "grid":
            with pytest.raises(hip_mod.SfwError) as e:
                g.knots(0, 1)
            assert e.value.status == SFW_ERR_STATE
        else:  # lists and sequences, host-staged or perturbed, read back
            k = g.knots(0, want[b][2])
            if b == "perturbed":
                assert _same(k, first)
            elif b == "seq":
                assert _same(k[:, 0], vx) and _same(k[:, 2], vth) and np.all(_bits(k[:, 1]) == 0)
            else:
                assert _same(k[0, 0], lx) and _same(k[0, 2], lth) and k.shape == (1, 3, 20)
            with pytest.raises(hip_mod.SfwError) as e:  # no normals were kept by any of them
                g.normals(0, 1)
            assert e.value.status == SFW_ERR_STATE
    # the scalar call consumes a perturbed stage
    stage["perturbed"]()
    g.score_one(rs, 0.3, 0.0, 0.1, scene.goal_args)
    with pytest.raises(hip_mod.SfwError) as e:
        g.launch()
    assert e.value.status == SFW_ERR_STATE
    with pytest.raises(hip_mod.SfwError) as e:
        g.knots(0, 1)
    assert e.value.status == SFW_ERR_STATE
    # timing and the points capture act on it as on a sequence stage
    g.set_timing(True)
    g.set_points_capture(True)
    stage["perturbed"]()
    g.launch()
    c, best, _ = g.fetch()
    assert _same(c, pc) and best == pb and g.last_launch_ms(0) >= 0.0
    pts = g.grid_points(best["index"])
    g.set_points_capture(False)
    g.set_timing(False)
    stage["perturbed"]()
    g.launch()
    g.fetch()
    assert _same(g.grid_points(best["index"]), pts)
    g.close()


# ---- 10. batch members ---------------------------------------------------------------------------------------------------------------
def test_batch_member_takes_its_own_path(hip_mod):
    scene = _scene((5, 12, 0))
    lin, ang = syn.reference_sampler()
    rs, ga = scene.robot_state, scene.goal_args
    nominal = _nominal(3)
    alone = _scorer(hip_mod, scene)
    want = [alone.score_perturbed(rs, 30, 21, nominal, SIGMA, WIDE[0], WIDE[1], (0, 7, 19), HOLO_GA, flags=KEEP)]
    knots, z = alone.knots(0, 30), alone.normals(0, 30)
    blend = alone.blend(L16, want_weights=True)
    want.append(alone.score_grid(rs, lin, ang, ga))
    alone.close()
    bs = hip_mod.BatchScorer(_params(), B=2)
    for i in range(2):
        bs.member(i).load_scene(scene)
    bs.member(0).stage_perturbed(rs, 30, 21, nominal, SIGMA, WIDE[0], WIDE[1], (0, 7, 19), HOLO_GA, flags=KEEP)
    bs.stage(1, rs, lin, ang, ga)
    bs.launch()
    bests = bs.fetch()
    for i in range(2):
        costs = bs.member(i).costs_view().copy()
        assert _same(costs, want[i][0]) and bests[i] == want[i][1], i
    d = bs.describe()
    assert d["members"] == 2 and d["one_launch_members"] == 1 and d["own_path_members"] == 1, d
    m = bs.member(0)
    assert _same(m.knots(0, 30), knots) and _same(m.normals(0, 30), z)
    got = m.blend(L16, want_weights=True)
    assert _same(got[1], blend[1]) and _same(got[2], blend[2]) and [s["eta"] for s in got[0]] == [s["eta"] for s in blend[0]]
    bs.close()


# ---- 11. plan_info --------------------------------------------------------------------------------------------------------------------
def test_plan_info_and_the_conservative_rest_flag(hip_mod):
    pinned, free = _scorer(hip_mod, _scene("pinned")), _scorer(hip_mod, _scene((5, 12, 0)))
    scene = _scene("pinned")
    listed = _scorer(hip_mod, scene)
    for n in (45, 257):
        _stage(pinned, scene, n, 3, 31)
        plan = pinned.plan_info()
        assert plan["samples"] == n and (n != 45 or plan["one_launch"] == 1)
        assert plan["levels"] == plan["split_step"] == plan["classes"] == plan["class_steps"] == 0
        assert plan["rest_noise_unreproduced"] == 1  # the box admits (0, 0): some sample may be commanded to rest
        k = pinned.knots(0, n)  # ... and every other field is what the same sequences report when the host stages them
        listed.stage_sequences(scene.robot_state, k[:, 0], k[:, 2], _knot_steps(3), HOLO_GA, vy=k[:, 1])
        assert {f: v for f, v in plan.items() if f != "rest_noise_unreproduced"} == \
            {f: v for f, v in listed.plan_info().items() if f != "rest_noise_unreproduced"}
    cases = [  # (box, flags) -> the flag with a pinned person
        (((0.0, -0.3, -0.5), (0.7, 0.3, 0.5)), 0, 1), (((0.0, 0.0, -0.5), (0.0, 0.0, 0.5)), 0, 1),
        (((0.05, -0.3, -0.5), (0.7, 0.3, 0.5)), 0, 0), (((-0.7, -0.3, -0.5), (-0.05, 0.3, 0.5)), 0, 0),
        (((0.0, 0.01, -0.5), (0.7, 0.3, 0.5)), 0, 0), (((0.0, -0.3, -0.5), (0.7, -0.01, 0.5)), 0, 0),
        (((0.0, 0.01, -0.5), (0.7, 0.3, 0.5)), NO_VY, 1), (((0.05, -0.3, -0.5), (0.7, 0.3, 0.5)), NO_VY, 0),
        (((0.0, -0.3, 0.1), (0.7, 0.3, 0.5)), 0, 1),  # (the angular channel takes no part)
    ]
    for box, flags, want in cases:
        _stage(pinned, scene, 45, 3, 32, flags, box)
        assert pinned.plan_info()["rest_noise_unreproduced"] == want, (box, flags)
        _stage(free, scene, 45, 3, 32, flags, box)  # nobody pinned: never
        assert free.plan_info()["rest_noise_unreproduced"] == 0
    # a robot alone (fewer than two agents): never
    base = _scene((5, 12, 0))
    alone = hip_mod.HipScorer(_params())
    alone.set_costmap(base.cells, base.origin_x, base.origin_y, base.resolution)
    alone.set_footprint(base.footprint)
    robot = (SfwAgent * 1)()
    C.memmove(C.byref(robot[0]), C.byref(base.agents[0]), C.sizeof(SfwAgent))
    alone.set_agents(robot)
    _stage(alone, base, 45, 3, 33)
    assert alone.plan_info()["rest_noise_unreproduced"] == 0
    for h in (pinned, free, listed, alone):
        h.close()
