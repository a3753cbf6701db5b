"""sfw_set_path on the device: the path term behind the rollout, against social_force_window_planner_amd/path.py.

Everything the term adds is a fixed IEEE sequence on the device's OWN Trajectory points (sfw_grid_points_batch), so every
comparison here is BIT FOR BIT: p against path.path_term on those points, the cost against off + w * p as float64 operations,
sentinels, captured terms and the selection.

Paths through the kernels (plan_info() says which one ran; with a path no stage is the one-launch kernel):
    small        sfw_rollout_small_kernel, then the term            k1abc      K1a (teams) + K1b + K1c, then the term: > 2048 samples
    k1abc_thr    the same with SFW_K1A_THREADS=1                    list_small, list_k1abc   the LIST instantiations, vy != 0
    sequence     two knots: the SEQ instantiation"""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import costmap_reference as CR
from sfw_test_util import _bits, _nominal, _np_best, _same, _workload
from sfw_test_util import _params as _scene_params
from social_force_window_planner_amd import path as P
from social_force_window_planner_amd._abi import (SFW_ERR_INVALID_ARG, SFW_ERR_STATE, SFW_PATH_MAX_POINTS, SFW_PRECISION_F32, SFW_PRECISION_F64,
                                                  SFW_PRECISION_F64_STRICT, SfwAgent, SfwPath, default_params)

pytestmark = pytest.mark.gpu

KPATHS = ["small", "k1abc", "k1abc_thr", "list_small", "list_k1abc", "sequence"]
WIDE = 2049  # more samples than the fused small-grid K1 takes
GEO = CR.geometry("wide_120x80_r0.05")
X0, Y0 = CR.mid_cell(GEO.origin_x, GEO.resolution, GEO.size_x), CR.mid_cell(GEO.origin_y, GEO.resolution, GEO.size_y)
LIN, ANG = np.linspace(0.0, 0.6, 5), np.linspace(-1.0, 1.0, 9)  # the 5 x 9 command set, with the grid's (0, 0) sample
DT = 0.1


def _polyline(n):
    """n path points near the robot: an arc bending left, with one repeated point from three points on"""
    if n == 1:
        return np.array([[X0 + 0.3, Y0 + 0.2]])
    s = np.linspace(0.0, 1.0, n)
    xy = np.stack([X0 - 0.1 + 0.7 * s, Y0 - 0.05 + 0.5 * s * s], axis=1)
    if n >= 3:
        xy[n // 2] = xy[n // 2 - 1]
    return xy


# (points of the path, steps of the rollout): S of 3 to 8, paths of 1, 2, 3 and 17 points
SHAPES = [(1, 3), (2, 5), (3, 8), (17, 6)]


def _map(walls=True):
    """a free map with a lethal block ahead and to the left of the robot's heading: the samples that turn left run into it"""
    cells = np.zeros((GEO.size_y, GEO.size_x), dtype=np.uint8)
    if walls:
        my, mx = np.mgrid[0:GEO.size_y, 0:GEO.size_x]
        cx, cy = GEO.origin_x + (mx + 0.5) * GEO.resolution, GEO.origin_y + (my + 0.5) * GEO.resolution
        cells[(np.hypot(cx - (X0 + 0.1), cy - (Y0 + 0.22)) < 0.1)] = 254
    return CR.make_map(cells, GEO.origin_x, GEO.origin_y, GEO.resolution)


RS = (X0, Y0, 0.7, 0.3, 0.0, 0.2)  # a non-zero heading
GOAL = (1.0, 0.7, 1.3, X0 + 1.0, Y0 + 0.4)


def _params(S, precision=SFW_PRECISION_F64):
    return default_params(sim_time=S * DT, sim_granularity=DT, precision=precision)


def _env(monkeypatch, kpath, fused="0"):
    monkeypatch.setenv("SFW_CYCLE_FUSED", fused)  # ("0": the path-off runs take the same kernels as the path-on ones)
    monkeypatch.setenv("SFW_K1A_THREADS", "1" if kpath == "k1abc_thr" else "0")


def _scorer(hip_mod, S, m=None, precision=SFW_PRECISION_F64, capture=False):
    """capture: sfw_set_points_capture — a launch that goes through the fused K1 leaves its own Trajectory points, and the
    distance, scan and add kernels run behind that capturing launch (force_alive, points and counts in pinned memory);
    without it (and for more than 2048 samples) the points come from a re-run of K1 into scratch buffers"""
    m = _map() if m is None else m
    g = hip_mod.HipScorer(_params(S, precision))
    g.set_points_capture(capture)
    g.set_costmap(m.cells, m.origin_x, m.origin_y, m.resolution)
    g.set_footprint(CR.FOOTPRINTS["point"])
    g.set_agents((SfwAgent * 0)())
    g.set_terms_capture(True)
    return g


def _launch(g, kpath):
    """one launch of the 5 x 9 command set through `kpath`: (costs, best, vx, vy, vth, skipped) — tiled to 2049 samples where
    the path asks for the K1a / K1b / K1c kernels"""
    nv, nw = len(LIN), len(ANG)
    n = nv * nw
    wide = kpath in ("k1abc", "k1abc_thr", "list_k1abc")
    k = -(-WIDE // n) if wide else 1
    idx = np.arange(k * n) % n
    vx, vth = np.repeat(LIN, nw)[idx], np.tile(ANG, nv)[idx]
    vy = None
    if kpath in ("small", "k1abc", "k1abc_thr"):
        costs, best = g.score_grid(RS, np.tile(LIN, k), ANG, GOAL)
        skipped = (vx == 0.0) & (vth == 0.0)
    elif kpath == "sequence":
        vy = 0.1 * np.cos(np.arange(len(idx)))
        costs, best = g.score_sequences(RS, np.stack([vx, vx[::-1]]), np.stack([vth, vth[::-1]]), (0, 2), GOAL, vy=np.stack([vy, -vy]))
        skipped = np.zeros(len(idx), dtype=bool)
    else:
        vy = 0.1 * np.cos(np.arange(len(idx)))  # a holonomic list: vy != 0
        costs, best = g.score_samples(RS, vx, vth, GOAL, vy=vy)
        skipped = np.zeros(len(idx), dtype=bool)
    info = g.plan_info()
    assert info["samples"] == len(idx) and info["chunks"] == 1 and (info["samples"] > 2048) == wide, info
    return np.array(costs), best, vx, vy, vth, skipped


def _points(g, T, S):
    """the device's own Trajectory points of all T samples (slices the fused K1 takes)"""
    pts, n = [], []
    for first in range(0, T, 1024):
        a, b = g.grid_points_batch(first, min(1024, T - first), S)
        pts.append(a)
        n.append(b)
    return np.concatenate(pts), np.concatenate(n)


_RUNS = {}


def _runs(hip_mod, monkeypatch, kpath, capture):
    """per (path points, steps): the path-off launch, the path-on launch and what the tests below compare — once per kernel path
    and capture setting"""
    _env(monkeypatch, kpath)
    if (kpath, capture) in _RUNS:
        return _RUNS[(kpath, capture)]
    out = []
    for n_pts, S in SHAPES:
        g = _scorer(hip_mod, S, capture=capture)
        xy, w = _polyline(n_pts), 2.5
        off, off_best, vx, vy, vth, skipped = _launch(g, kpath)
        assert g.plan_info()["one_launch"] == 0  # (SFW_CYCLE_FUSED=0)
        off_terms = g.cost_terms()
        with pytest.raises(hip_mod.SfwError) as e:
            g.path_term(0, len(off))  # the staged grid has no path
        assert e.value.status == SFW_ERR_STATE
        g.set_path(xy, w)
        on, on_best, *_ = _launch(g, kpath)
        assert g.plan_info()["one_launch"] == 0
        on_terms = g.cost_terms()
        p = g.path_term(0, len(on)).copy()
        pts, n_points = _points(g, len(on), S)
        g.set_path(None)
        again, again_best, *_ = _launch(g, kpath)
        again_terms = g.cost_terms()
        g.close()
        out.append(dict(n_pts=n_pts, S=S, xy=xy, w=w, off=off, off_best=off_best, off_terms=off_terms, on=on, on_best=on_best,
                        on_terms=on_terms, p=p, pts=pts, n_points=n_points, again=again, again_best=again_best,
                        again_terms=again_terms, vx=vx, vy=vy, vth=vth, skipped=skipped))
    _RUNS[(kpath, capture)] = out
    return out


# ---- 1. the exact term: the test that fails without the feature -----------------------------------------------------------------------
@pytest.mark.parametrize("capture", [True, False], ids=["capture", "rerun"])
@pytest.mark.parametrize("kpath", KPATHS)
def test_exact_term(hip_mod, monkeypatch, kpath, capture):
    """capture: with points capture on, p against the points of the very launch that produced it (the routes of at most 2048
    samples; a larger launch does not capture and its points come from the re-run, as with capture off)"""
    rejected_somewhere = False
    for r in _runs(hip_mod, monkeypatch, kpath, capture):
        S, T = r["S"], len(r["on"])
        assert r["pts"].shape == (T, S, 3)
        want = P.path_term(r["pts"], r["n_points"], r["xy"])
        want = np.where(r["skipped"], P.SFW_COST_SKIPPED, want)
        assert _same(r["p"], want), (kpath, r["n_pts"], S, np.flatnonzero(_bits(r["p"]) != _bits(want))[:8])
        # costmap-rejected samples carry SFW_COST_INVALID, the grid's (0, 0) sample SFW_COST_SKIPPED, everyone else a term
        rejected = (r["off"] == -1.0)
        assert np.array_equal(r["p"] == -1.0, rejected) and np.array_equal(r["p"] == -2.0, r["skipped"])
        assert np.array_equal(r["n_points"] < S, rejected | r["skipped"])
        valid = ~rejected & ~r["skipped"]
        assert np.all(r["p"][valid] > 0.0) and np.all(np.isfinite(r["p"][valid]))
        assert r["skipped"].any() == (kpath in ("small", "k1abc", "k1abc_thr")) and valid.sum() >= T // 4
        rejected_somewhere |= bool(rejected.any())
        # pose 0 is the robot's own pose in every sample, at a non-zero heading
        assert np.all(r["pts"][valid, 0, 0] == RS[0]) and np.all(r["pts"][valid, 0, 2] == RS[2])
        assert len({b for b in _bits(r["p"][valid]).tolist()}) >= 10  # (the term tells the samples apart)
    assert rejected_somewhere


# ---- 2. the exact cost ---------------------------------------------------------------------------------------------------------------
def _assert_cost(r, what):
    on, off, p, w = r["on"], r["off"], r["p"], r["w"]
    want = P.add(off, p, w)  # off + w * p as float64 operations where off is no sentinel
    assert _same(on, want), (what, np.flatnonzero(_bits(on) != _bits(want))[:8])
    sentinel = off < 0.0
    assert _same(on[sentinel], off[sentinel]) and np.all(on[~sentinel] == off[~sentinel] + np.float64(w) * p[~sentinel])
    assert np.any(on[~sentinel] != off[~sentinel])
    assert _same(r["on_terms"], r["off_terms"]), what  # the captured five terms do not change
    nb = _np_best(on, r["vx"], r["vy"], r["vth"])
    best = r["on_best"]
    assert best["index"] == nb["index"] and best["cost"] == nb["cost"] and best["n_valid"] == nb["n_valid"], (what, best, nb)
    assert (best["vx"], best["vtheta"]) == (nb["vx"], nb["vtheta"])
    # ... and set_path(None) restores the path-off result bit for bit
    assert _same(r["again"], off) and _same(r["again_terms"], r["off_terms"]) and r["again_best"] == r["off_best"], what


@pytest.mark.parametrize("capture", [True, False], ids=["capture", "rerun"])
@pytest.mark.parametrize("kpath", KPATHS)
def test_exact_cost(hip_mod, monkeypatch, kpath, capture):
    for r in _runs(hip_mod, monkeypatch, kpath, capture):
        _assert_cost(r, (kpath, capture, r["n_pts"], r["S"]))


def test_one_launch_flag_under_default_settings(hip_mod, monkeypatch):
    monkeypatch.delenv("SFW_CYCLE_FUSED", raising=False)
    g = _scorer(hip_mod, 5)
    off, _ = g.score_grid(RS, LIN, ANG, GOAL)
    assert g.plan_info()["one_launch"] == 1
    g.set_path(_polyline(3), 1.0)
    on, _ = g.score_grid(RS, LIN, ANG, GOAL)
    assert g.plan_info()["one_launch"] == 0
    p = g.path_term(0, len(on))
    assert _same(on, P.add(off, p, 1.0))  # (the path-off run was the one-launch kernel: the same costs from other kernels)
    g.set_path(None)
    again, _ = g.score_grid(RS, LIN, ANG, GOAL)
    assert g.plan_info()["one_launch"] == 1 and _same(again, off)
    g.close()


@pytest.mark.parametrize("precision", [SFW_PRECISION_F32, SFW_PRECISION_F64_STRICT])
def test_precision_modes_do_not_reach_the_term(hip_mod, monkeypatch, precision):
    """the term is the robot's: SFW_PRECISION_F32 and the strict mode change the pedestrians' arithmetic only"""
    _env(monkeypatch, "small")
    scene = _people_scene()
    xy = _people_path(scene)
    res = {}
    for prec in (SFW_PRECISION_F64, precision):
        g = hip_mod.HipScorer(_scene_params(prec))
        g.load_scene(scene)
        g.set_terms_capture(True)
        lin, ang = np.linspace(0.0, 0.7, 5), np.linspace(-0.5, 0.5, 9)
        off, _ = g.score_grid(scene.robot_state, lin, ang, scene.goal_args)
        off_terms = g.cost_terms()
        g.set_path(xy, 3.0)
        on, best = g.score_grid(scene.robot_state, lin, ang, scene.goal_args)
        p = g.path_term(0, len(on)).copy()
        assert _same(on, P.add(off, p, 3.0)) and _same(g.cost_terms(), off_terms)
        nb = _np_best(on, np.repeat(lin, len(ang)), None, np.tile(ang, len(lin)))
        assert best["index"] == nb["index"] and best["cost"] == nb["cost"]
        res[prec] = p
        g.close()
    assert _same(res[precision], res[SFW_PRECISION_F64]) and (res[precision] > 0).any()


# ---- 3. with pedestrians ---------------------------------------------------------------------------------------------------------------
def _people_scene(n_people=3, contact=True):
    """a one-second scene (32 steps) with three people; person 1 stands 0.9 m ahead of the robot, where the fastest samples
    touch it"""
    from social_force_window_planner_amd import synthetic as syn
    base = syn.make_scene(_workload(n_people, 31, 0))
    agents = (type(base.agents[0]) * len(base.agents))()
    for a in range(len(base.agents)):
        C.memmove(C.byref(agents[a]), C.byref(base.agents[a]), C.sizeof(agents[a]))
    if contact:
        q = agents[1]
        q.x, q.y, q.vx, q.vy, q.has_goal, q.desired_velocity = base.robot_state[0] + 0.9, base.robot_state[1], 0.0, 0.0, 0, 0.0
    return dataclasses.replace(base, cells=np.zeros_like(base.cells), agents=agents)


def _people_path(scene):
    x, y = scene.robot_state[0], scene.robot_state[1]
    return np.array([[x - 0.2, y - 0.1], [x + 0.4, y + 0.1], [x + 0.4, y + 0.1], [x + 0.8, y + 0.5]])


@pytest.mark.parametrize("capture", [True, False], ids=["capture", "rerun"])
@pytest.mark.parametrize("fused", ["0", "1"])
def test_with_pedestrians(hip_mod, monkeypatch, fused, capture):
    """capture: the term's kernels behind a capturing launch (force_alive: K2 also integrates what the costmap rejected) — the
    contact-rejected samples keep their p, taken from the points of that launch"""
    _env(monkeypatch, "small", fused)
    scene = _people_scene()
    S, w = 32, 1.75
    g = hip_mod.HipScorer(_scene_params())
    g.load_scene(scene)
    g.set_terms_capture(True)
    g.set_points_capture(capture)
    lin, ang = np.linspace(0.0, 0.7, 5), np.linspace(-0.5, 0.5, 9)
    off, _ = g.score_grid(scene.robot_state, lin, ang, scene.goal_args)
    off_terms = g.cost_terms()
    g.set_path(_people_path(scene), w)
    on, best = g.score_grid(scene.robot_state, lin, ang, scene.goal_args)
    assert g.plan_info()["one_launch"] == 0
    T = len(on)
    p = g.path_term(0, T).copy()
    pts, n_points = g.grid_points_batch(0, T, S)
    skipped = off == -2.0
    contact = (off == -1.0)  # (a free map: every rejection is a pedestrian contact)
    assert contact.sum() >= 3 and np.all(n_points[contact] < S) and (~contact & ~skipped).sum() >= 20
    # the term of EVERY scored sample — the contact-rejected ones included — from all S of the device's points
    want = np.where(skipped, -2.0, P.path_term(pts, None, _people_path(scene)))
    assert _same(p, want)
    assert np.all(on[contact] == -1.0) and np.all(np.isfinite(p[contact])) and np.all(p[contact] > 0.0)
    assert _same(on, P.add(off, p, w)) and _same(g.cost_terms(), off_terms)
    nb = _np_best(on, np.repeat(lin, len(ang)), None, np.tile(ang, len(lin)))
    assert best["index"] == nb["index"] and best["cost"] == nb["cost"] and best["n_valid"] == nb["n_valid"]
    # score_one and score_one_crowd give the grid's entry, the term included
    for t in (int(best["index"]), int(np.flatnonzero(contact)[0])):
        vx, vth = float(lin[t // len(ang)]), float(ang[t % len(ang)])
        assert _same(g.score_one(scene.robot_state, vx, 0.0, vth, scene.goal_args)[0], on[t])
        assert _same(g.score_one_crowd(scene.robot_state, vx, 0.0, vth, scene.goal_args)["cost"], on[t])
    g.close()


def test_with_pedestrians_prefix_levels(hip_mod):
    """a grid large enough for the shared-prefix levels: the term runs on the side stream beside them"""
    scene = _people_scene(20, contact=False)
    g = hip_mod.HipScorer(_scene_params())
    g.load_scene(scene)
    lin, ang = np.linspace(0.0, 0.7, 96), np.linspace(-0.5, 0.5, 96)
    off, _ = g.score_grid(scene.robot_state, lin, ang, scene.goal_args)
    assert g.plan_info()["levels"] > 0
    g.set_path(_people_path(scene), 0.5)
    on, best = g.score_grid(scene.robot_state, lin, ang, scene.goal_args)
    assert g.plan_info()["levels"] > 0
    p = g.path_term(0, len(on)).copy()
    assert _same(on, P.add(off, p, 0.5)) and (on != off).any()
    # p itself against numpy on the device's points (a free map: every rejection is a contact, and such a sample keeps its p)
    pts, _ = _points(g, len(on), 32)
    assert _same(p, np.where(off == -2.0, -2.0, P.path_term(pts, None, _people_path(scene))))
    assert np.all(p[off != -2.0] > 0)
    nb = _np_best(on, np.repeat(lin, len(ang)), None, np.tile(ang, len(lin)))
    assert best["index"] == nb["index"]
    g.close()


# ---- 4. chunks ---------------------------------------------------------------------------------------------------------------------------
def test_chunks(hip_mod, monkeypatch):
    """SFW_TABLE_BUDGET_MB=1 (26 B per step and sample with a path).  At 20 steps: chunks of 2016 samples of a 64 x 33 grid, each
    through the fused small K1 at chunk_begin != 0.  At 8 steps: chunks of 5041 samples of a 64 x 99 grid, too large for the
    fused K1, so the term runs behind K1a + K1b + K1c at chunk_begin != 0.  Bit-identical to one chunk."""
    monkeypatch.setenv("SFW_CYCLE_FUSED", "0")
    lin = np.linspace(0.05, 0.65, 64)
    xy = _polyline(17)

    def run(S, ang):
        g = _scorer(hip_mod, S)
        g.set_path(xy, 1.5)
        costs, best = g.score_grid(RS, lin, ang, GOAL)
        out = (np.array(costs), g.path_term(0, len(costs)).copy(), best, g.plan_info())
        g.close()
        return out
    for S, ang in ((20, np.linspace(-1.0, 1.0, 33)), (8, np.linspace(-1.0, 1.0, 99))):
        one = run(S, ang)
        assert one[3]["chunks"] == 1 and (one[0] == -1.0).any() and (one[0] >= 0).any()
        monkeypatch.setenv("SFW_TABLE_BUDGET_MB", "1")
        many = run(S, ang)
        monkeypatch.delenv("SFW_TABLE_BUDGET_MB")
        assert many[3]["chunks"] >= 2, many[3]
        assert (many[3]["samples"] / many[3]["chunks"] > 2048) == (S == 8), many[3]
        assert _same(many[0], one[0]) and _same(many[1], one[1]) and many[2] == one[2]


def test_table_budget_counts_the_distance_table(hip_mod, monkeypatch):
    """8 B per step and sample join the 18 B of the K1 tables in what SFW_TABLE_BUDGET_MB chunks: at 8 steps and 2 MB, 14 563
    samples fit without a path (one chunk of the 100 x 120 grid) and 10 082 with one (two chunks)"""
    monkeypatch.setenv("SFW_CYCLE_FUSED", "0")
    monkeypatch.setenv("SFW_TABLE_BUDGET_MB", "2")
    g = _scorer(hip_mod, 8)
    lin, ang = np.linspace(0.05, 0.65, 100), np.linspace(-1.0, 1.0, 120)
    g.stage(RS, lin, ang, GOAL)
    assert g.plan_info()["chunks"] == 1
    g.set_path(_polyline(2), 1.0)
    g.stage(RS, lin, ang, GOAL)
    assert g.plan_info()["chunks"] == 2
    g.close()


def test_long_path_is_sliced_over_the_grid(hip_mod, monkeypatch):
    """A path of more than 128 segments under a launch of at most 65 536 poses: the distance kernel walks slices of 64 segments
    in the grid's z and the slices meet by an integer atomicMin on the bit pattern.  Bit-identical to one thread per pose
    (SFW_PATH_SLICES=0) and to numpy, through the fused K1 and through K1a + K1b + K1c; a repeated point and a path that ends
    inside a slice among the 199 / 1023 segments."""
    for kpath, n_pts, S in (("small", 200, 8), ("list_k1abc", 200, 6), ("small", 1024, 5)):
        _env(monkeypatch, kpath)
        s = np.linspace(0.0, 1.0, n_pts)
        xy = np.stack([X0 - 0.2 + 1.1 * s, Y0 - 0.1 + 0.6 * s * s + 0.02 * np.sin(40.0 * s)], axis=1)
        xy[n_pts // 3] = xy[n_pts // 3 - 1]
        res = {}
        for slices in ("1", "0"):
            monkeypatch.setenv("SFW_PATH_SLICES", slices)
            g = _scorer(hip_mod, S)
            g.set_path(xy, 1.5)
            costs, best, *_ = _launch(g, kpath)
            p = g.path_term(0, len(costs)).copy()
            pts, n_points = _points(g, len(costs), S)
            g.close()
            res[slices] = (costs, p, best)
            skipped = costs == -2.0
            assert _same(p, np.where(skipped, -2.0, P.path_term(pts, n_points, xy))), (kpath, n_pts, slices)
        monkeypatch.delenv("SFW_PATH_SLICES")
        assert _same(res["1"][0], res["0"][0]) and _same(res["1"][1], res["0"][1]) and res["1"][2] == res["0"][2]
        assert (res["1"][1] > 0).any() and (res["1"][1] == -1.0).any()


# ---- 5. together with the stop check ---------------------------------------------------------------------------------------------------
def test_with_the_stop_check(hip_mod, monkeypatch):
    _env(monkeypatch, "small")
    # a lethal ring 0.8 m around the robot: beyond every rollout (0.48 m at most), inside the braking path of the faster samples
    cells = np.zeros((GEO.size_y, GEO.size_x), dtype=np.uint8)
    my, mx = np.mgrid[0:GEO.size_y, 0:GEO.size_x]
    d = np.hypot(GEO.origin_x + (mx + 0.5) * GEO.resolution - X0, GEO.origin_y + (my + 0.5) * GEO.resolution - Y0)
    cells[(d > 0.8) & (d < 0.9)] = 254
    m = CR.make_map(cells, GEO.origin_x, GEO.origin_y, GEO.resolution)
    S, w, xy = 8, 2.0, _polyline(3)
    g = _scorer(hip_mod, S, m)
    g.set_stop_check((0.3, 0.3, 1.0, 256))
    off, _ = g.score_grid(RS, LIN, ANG, GOAL)
    off_terms = g.cost_terms()
    _, hit = g.stop_info(0, len(off))
    g.set_path(xy, w)
    on, best = g.score_grid(RS, LIN, ANG, GOAL)
    p = g.path_term(0, len(on)).copy()
    _, hit_on = g.stop_info(0, len(on))
    assert np.array_equal(hit, hit_on)
    stopped = hit >= 0
    skipped = off == -2.0
    assert np.array_equal(stopped, off == -1.0)  # (no rollout pose is illegal in this scene: every rejection is the tail's)
    assert stopped.sum() >= 3 and (~stopped & ~skipped).sum() >= 10
    # the samples the tail rejects get the sentinel; the survivors their term and cost
    assert np.all(p[stopped] == -1.0) and np.all(on[stopped] == -1.0) and np.all(p[skipped] == -2.0)
    pts, n_points = g.grid_points_batch(0, len(on), S)
    assert np.all(n_points[stopped] == S)  # (rejected behind S legal poses)
    want = P.path_term(pts, n_points, xy)
    live = ~stopped & ~skipped
    assert _same(p[live], want[live]) and _same(on, P.add(off, p, w)) and _same(g.cost_terms(), off_terms)
    nb = _np_best(on, np.repeat(LIN, len(ANG)), None, np.tile(ANG, len(LIN)))
    assert best["index"] == nb["index"] and best["cost"] == nb["cost"] and not stopped[best["index"]]
    g.close()


# ---- 6. re-score -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kpath", ["small", "list_small"])
def test_rescore(hip_mod, monkeypatch, kpath):
    _env(monkeypatch, kpath)
    S, xy = 6, _polyline(17)
    g = _scorer(hip_mod, S)
    prm = g.params
    w5 = (prm.vel_weight, prm.distance_weight, prm.angle_weight, prm.costmap_weight, prm.social_weight)
    g.set_path(xy, 2.5)
    on, on_best, vx, vy, vth, _ = _launch(g, kpath)
    # rescore(w) with a path staged is what the launch returned, and with other weights what such a launch would
    bests, costs = g.rescore([w5, (0.3, 2.0, 0.1, 0.5, 1.0)], want_costs=True)
    assert _same(costs[0], on) and bests[0] == on_best
    # rescore_path: three path weights — 0 and a negative one among them — over the one launch, field for field what three
    # launches return
    pws = (0.0, 2.5, -0.75)
    sweep, sweep_costs = g.rescore_path(w5, pws, want_costs=True)
    staged, staged_costs = g.rescore_path(w5, None, K=2, want_costs=True)
    assert _same(staged_costs[0], on) and _same(staged_costs[1], on) and staged[0] == staged[1] == on_best
    p = g.path_term(0, len(on)).copy()
    for k, pw in enumerate(pws):
        g.set_path(xy, pw)
        c, b, *_ = _launch(g, kpath)
        assert _same(sweep_costs[k], c) and sweep[k] == b, (k, pw, sweep[k], b)
        assert _same(g.path_term(0, len(c)), p)
    assert not _same(sweep_costs[0], sweep_costs[2])
    # the second weight vector of rescore() against a launch under those weights
    g.set_params(dataclasses_replace_weights(prm, (0.3, 2.0, 0.1, 0.5, 1.0)))
    g.set_path(xy, 2.5)
    c, b, *_ = _launch(g, kpath)
    assert _same(costs[1], c) and bests[1] == b
    # without a path: rescore_path is refused, rescore is the five terms
    g.set_path(None)
    c, b, *_ = _launch(g, kpath)
    with pytest.raises(hip_mod.SfwError) as e:
        g.rescore_path(w5, pws)
    assert e.value.status == SFW_ERR_STATE
    for bad in ((math.nan, 1.0), (1.0, math.inf)):
        g.set_path(xy, 1.0)
        _launch(g, kpath)
        with pytest.raises(hip_mod.SfwError) as e:
            g.rescore_path(w5, bad)
        assert e.value.status == SFW_ERR_INVALID_ARG
    g.close()


def dataclasses_replace_weights(prm, w):
    """a copy of the parameters under other weights"""
    q = type(prm)()
    C.memmove(C.byref(q), C.byref(prm), C.sizeof(prm))
    q.vel_weight, q.distance_weight, q.angle_weight, q.costmap_weight, q.social_weight = w
    return q


# ---- 7. ensembles ------------------------------------------------------------------------------------------------------------------------
def _hypotheses(scene, M):
    """M crowds: the scene's, and copies with person 2 shifted — hypothesis 0 alone keeps the contact person in the robot's way"""
    out = []
    for m in range(M):
        agents = (type(scene.agents[0]) * len(scene.agents))()
        for a in range(len(scene.agents)):
            C.memmove(C.byref(agents[a]), C.byref(scene.agents[a]), C.sizeof(agents[a]))
        if m > 0:
            agents[1].y += 2.0 + m
            agents[2].x += 0.1 * m
        out.append(agents)
    return out


@pytest.mark.parametrize("kind", ["grid", "sequences"])
def test_ensemble(hip_mod, kind):
    scene = _people_scene()
    M, w, xy = 3, 1.25, _people_path(scene)
    e = hip_mod.EnsembleScorer(_scene_params(), 0, M)
    e.load_scene(scene, _hypotheses(scene, M))
    lin, ang = np.linspace(0.0, 0.7, 5), np.linspace(-0.5, 0.5, 9)
    vx, vth = np.repeat(lin, len(ang)), np.tile(ang, len(lin))
    vy = 0.05 * np.cos(np.arange(len(vx)))
    probs = (0.2, 0.5, 0.3)

    def score(mode):
        if kind == "grid":
            return e.score_grid(scene.robot_state, lin, ang, scene.goal_args, mode=mode, probs=probs)
        return e.score_sequences(scene.robot_state, np.stack([vx, vx]), np.stack([vth, vth[::-1]]), (0, 9), scene.goal_args,
                                 vy=np.stack([vy, -vy]), mode=mode, probs=probs)
    settings = [("mean", None), ("max", None), ("mean", (0.5, 0.25))]  # the last: a risk with contact_mass > 0
    off = {}
    for mode, risk in settings:
        if risk:
            e.set_risk(tail_mass=risk[0], contact_mass=risk[1])
        c, rej, _ = score(mode)
        off[(mode, risk)] = (np.array(c), np.array(rej))
        e.set_risk()
    e.set_path(xy, w)
    for m in range(M):
        got = e.member(m).path()
        assert _same(got[0], xy) and got[1] == w
    saw_contact_accept = False
    for mode, risk in settings:
        if risk:
            e.set_risk(tail_mass=risk[0], contact_mass=risk[1])
        c, rej, best = score(mode)
        c, rej = np.array(c), np.array(rej)
        T = len(c)
        ps = [e.member(m).path_term(0, T).copy() for m in range(M)]
        assert all(_same(ps[m], ps[0]) for m in range(M))  # the same robot, map and path: the same p in every member
        o, o_rej = off[(mode, risk)]
        assert np.array_equal(rej, o_rej)
        assert _same(c, P.add(o, ps[0], w)), (kind, mode, risk)
        assert (c != o).any()
        nb = _np_best(c, vx, vy if kind == "sequences" else None, vth)
        assert best["index"] == nb["index"] and best["cost"] == nb["cost"]
        # re-aggregated without a rollout: the same vector
        c2, rej2, best2 = e.aggregate(mode=mode, probs=probs)
        assert _same(c2, c) and best2 == best
        if risk:  # a sample member 0 rejects by contact, accepted under the bound, has member 0's p in its cost
            acc = (rej > 0) & (c >= 0)
            saw_contact_accept |= bool(acc.any())
            assert np.all(np.isfinite(ps[0][acc])) and np.all(ps[0][acc] > 0)
        e.set_risk()
    # (the grid's fastest samples touch hypothesis 0's person whatever their angular target; the sequences may or may not)
    assert saw_contact_accept or kind == "sequences"
    # differing member settings: the scoring call is refused
    e.member(1).set_path(xy, w + 1.0)
    with pytest.raises(hip_mod.SfwError) as err:
        score("mean")
    assert err.value.status == SFW_ERR_STATE
    e.member(1).set_path(None)
    with pytest.raises(hip_mod.SfwError) as err:
        score("mean")
    assert err.value.status == SFW_ERR_STATE
    e.set_path(None)
    c, rej, _ = score("mean")
    assert _same(c, off[("mean", None)][0])
    e.close()


# ---- 8. MPPI -----------------------------------------------------------------------------------------------------------------------------
def test_mppi_run_equals_the_loop_of_single_calls(hip_mod):
    """three iterations of the chain against its definition, call by call (as tests/test_mppi_gpu.py), with a path on"""
    scene = _people_scene()
    K, n, seed, lam, gamma, I = 4, 64, 5, 0.5, 0.1, 3
    nominal, sigma, lo, hi = _nominal(K), (0.15, 0.05, 0.3), (0.0, -0.3, -0.5), (0.7, 0.3, 0.5)
    ks, ga = (0, 5, 11, 19), (1.0, 1.0, 1.0, scene.goal_args[3], scene.goal_args[4])
    xy, w = _people_path(scene), 4.0

    def scorer(path=True):
        g = hip_mod.HipScorer(_scene_params())
        g.load_scene(scene)
        if path:
            g.set_path(xy, w)
        return g
    a, b, plain = scorer(), scorer(), scorer(False)
    stats, plans, best = a.mppi_run(scene.robot_state, n, seed, nominal, sigma, lo, hi, ks, ga, I, lam, gamma)
    nom, w_stats, w_plans, w_best = np.array(nominal, dtype=np.float64), [], [], None
    for i in range(I):
        b.stage_perturbed(scene.robot_state, n, seed + i, nom, sigma, lo, hi, ks, ga)
        b.launch()
        _, w_best, _ = b.fetch(want_costs=False)
        st, u, _ = b.blend([lam], gamma=gamma)
        if st[0]["n_valid"] > 0:
            nom = u[0].copy()
        w_stats.append(st[0])
        w_plans.append(nom.copy())
    assert _same(plans, np.stack(w_plans)) and best == w_best
    assert [sorted((k, _bits(float(v)).item()) for k, v in d.items()) for d in stats] == \
        [sorted((k, _bits(float(v)).item()) for k, v in d.items()) for d in w_stats]
    ca, cb = a.fetch()[0].copy(), b.fetch()[0].copy()
    assert _same(ca, cb) and _same(a.path_term(0, n), b.path_term(0, n))
    # ... and the path does steer the chain: other plans than without it
    _, plain_plans, _ = plain.mppi_run(scene.robot_state, n, seed, nominal, sigma, lo, hi, ks, ga, I, lam, gamma)
    assert not _same(plans, plain_plans)
    for g in (a, b, plain):
        g.close()


def test_ensemble_mppi_run_equals_the_loop_of_single_calls(hip_mod):
    scene = _people_scene()
    M, K, n, seed, lam, gamma, I = 3, 4, 64, 7, 0.5, 0.1, 3
    nominal, sigma, lo, hi = _nominal(K), (0.15, 0.05, 0.3), (0.0, -0.3, -0.5), (0.7, 0.3, 0.5)
    ks, ga = (0, 5, 11, 19), (1.0, 1.0, 1.0, scene.goal_args[3], scene.goal_args[4])
    xy, w = _people_path(scene), 4.0

    def ensemble():
        e = hip_mod.EnsembleScorer(_scene_params(), 0, M)
        e.load_scene(scene, _hypotheses(scene, M))
        e.set_path(xy, w)
        return e
    a, b = ensemble(), ensemble()
    stats, plans, best, costs, rej = a.mppi_run(scene.robot_state, n, seed, nominal, sigma, lo, hi, ks, ga, I, lam, gamma, mode="max",
                                                want_costs=True)
    nom, w_stats, w_plans = np.array(nominal, dtype=np.float64), [], []
    for i in range(I):
        wc, wr, w_best = b.score_perturbed(scene.robot_state, n, seed + i, nom, sigma, lo, hi, ks, ga, mode="max")
        st, u, _ = b.blend([lam], gamma=gamma)
        if st[0]["n_valid"] > 0:
            nom = u[0].copy()
        w_stats.append(st[0])
        w_plans.append(nom.copy())
    assert _same(plans, np.stack(w_plans)) and best == w_best and _same(costs, wc) and np.array_equal(rej, wr)
    assert [sorted((k, _bits(float(v)).item()) for k, v in d.items()) for d in stats] == \
        [sorted((k, _bits(float(v)).item()) for k, v in d.items()) for d in w_stats]
    # the last iteration's costs carry the term: the aggregate without it differs by w * p
    p = a.member(0).path_term(0, n).copy()
    a.set_path(None)  # (read by the next stage: the re-aggregation still sees the staged path)
    c2, _, _ = a.aggregate(mode="max")
    assert _same(c2, costs) and np.all(p[np.array(costs) >= 0] > 0)
    a.close()
    b.close()


# ---- 9. batches --------------------------------------------------------------------------------------------------------------------------
def test_batch_member_with_a_path_takes_its_own_path(hip_mod, monkeypatch):
    monkeypatch.setenv("SFW_CYCLE_FUSED", "1")
    S, xy, w = 5, _polyline(3), 2.0
    m = _map()

    def load(h):
        h.set_params(_params(S))
        h.set_costmap(m.cells, m.origin_x, m.origin_y, m.resolution)
        h.set_footprint(CR.FOOTPRINTS["point"])
        h.set_agents((SfwAgent * 0)())
    states = [RS, (X0 + 0.1, Y0, 0.2, 0.1, 0.0, 0.0), (X0, Y0 - 0.1, -0.4, 0.4, 0.0, -0.1)]

    def batch(with_path):
        bs = hip_mod.BatchScorer(_params(S), 0, 3)
        for i in range(3):
            load(bs.member(i))
            if i == 1 and with_path:
                bs.member(i).set_path(xy, w)
            bs.stage(i, states[i], LIN, ANG, GOAL)
        bs.launch()
        bests = bs.fetch()
        out = (bests, [np.array(bs._costs(i)) for i in range(3)], bs.describe(),
               bs.member(1).path_term(0, len(LIN) * len(ANG)).copy() if with_path else None)
        bs.close()
        return out
    plain, mixed = batch(False), batch(True)
    assert plain[2]["one_launch_members"] == 3 and plain[2]["own_path_members"] == 0, plain[2]
    assert mixed[2]["one_launch_members"] == 2 and mixed[2]["own_path_members"] == 1, mixed[2]
    for i in (0, 2):  # the other members: bit-identical to a batch without the path
        assert _same(mixed[1][i], plain[1][i]) and mixed[0][i] == plain[0][i]
    s = _scorer(hip_mod, S)
    s.set_path(xy, w)
    costs, best = s.score_grid(states[1], LIN, ANG, GOAL)
    assert _same(mixed[1][1], costs) and mixed[0][1] == best and _same(mixed[3], s.path_term(0, len(costs)))
    assert _same(mixed[1][1], P.add(plain[1][1], mixed[3], w)) and (mixed[1][1] != plain[1][1]).any()
    s.close()


# ---- 10. behaviour -----------------------------------------------------------------------------------------------------------------------
def test_l_shaped_plan(hip_mod):
    """An L-shaped plan — 1 m ahead, then 1 m to the left — with the way-point beyond the corner, on a free map without agents.
    Without the term the winner cuts the corner (it turns towards the way-point at once and leaves the plan); with a heavily
    weighted term the winner is the sample whose mean D is smallest."""
    m = _map(walls=False)
    S = 8
    g = hip_mod.HipScorer(default_params(sim_time=2.0, sim_granularity=0.25))
    g.set_costmap(m.cells, m.origin_x, m.origin_y, m.resolution)
    g.set_footprint(CR.FOOTPRINTS["point"])
    g.set_agents((SfwAgent * 0)())
    rs = (X0 - 0.5, Y0 - 0.5, 0.0, 0.4, 0.0, 0.0)  # on the first leg, heading along it
    xy = np.array([[X0 - 0.5, Y0 - 0.5], [X0 + 0.5, Y0 - 0.5], [X0 + 0.5, Y0 + 0.5]])
    goal = (2.0, 0.0, 3.0, X0 + 0.5, Y0 + 0.3)  # the way-point: beyond the corner, on the second leg
    lin, ang = np.linspace(0.1, 0.5, 5), np.linspace(-1.0, 1.0, 9)
    vx, vth = np.repeat(lin, len(ang)), np.tile(ang, len(lin))
    off, off_best = g.score_grid(rs, lin, ang, goal)
    g.set_path(xy, 1e4)
    on, on_best = g.score_grid(rs, lin, ang, goal)
    p = g.path_term(0, len(on)).copy()
    pts, n_points = g.grid_points_batch(0, len(on), S)
    g.close()
    assert np.all(off >= 0) and np.all(n_points == S) and _same(p, P.path_term(pts, n_points, xy))
    # without the term: the winner leaves the plan towards the way-point (a left turn), and is not the sample nearest to the plan
    t_off = _np_best(off, vx, None, vth)["index"]
    assert off_best["index"] == t_off and vth[t_off] > 0 and p[t_off] > p.min()
    # with it: the sample whose mean D is smallest (numpy's selection over the returned vectors agrees with the device's)
    t_on = _np_best(on, vx, None, vth)["index"]
    assert on_best["index"] == t_on and t_on != t_off
    assert p[t_on] == p.min() and p[t_on] < p[t_off] and vth[t_on] == 0.0


# ---- state and errors ---------------------------------------------------------------------------------------------------------------------
def test_state_and_errors(hip_mod, monkeypatch):
    monkeypatch.setenv("SFW_CYCLE_FUSED", "1")
    g = _scorer(hip_mod, 5)
    L = hip_mod.lib()
    assert g.path() is None
    n, w, on = C.c_int32(9), C.c_double(9.0), C.c_int32(9)
    assert L.sfw_get_path(g._h, None, 0, C.byref(n), C.byref(w), C.byref(on)) == 0 and (n.value, w.value, on.value) == (0, 0.0, 0)
    good = _polyline(3)
    g.set_path(good, -0.5)  # a negative weight is accepted
    got = g.path()
    assert _same(got[0], good) and got[1] == -0.5
    big = np.zeros((SFW_PATH_MAX_POINTS + 1, 2))

    def raw(xy, n_points, reserved, weight):
        xy = np.ascontiguousarray(xy, dtype=np.float64)
        return SfwPath(xy.ctypes.data_as(C.POINTER(C.c_double)), n_points, reserved, weight), xy
    bads = [raw(good, 0, 0, 1.0), raw(good, -1, 0, 1.0), raw(big, SFW_PATH_MAX_POINTS + 1, 0, 1.0), raw(good, 3, 1, 1.0),
            raw(good, 3, 0, math.nan), raw(good, 3, 0, math.inf), raw([[0.0, math.nan]], 1, 0, 1.0), raw([[math.inf, 0.0]], 1, 0, 1.0),
            raw([[0.0, 0.0], [1.0000001e7, 0.0]], 2, 0, 1.0), raw([[0.0, -1.0000001e7]], 1, 0, 1.0)]
    for bad, _keep in bads:
        assert L.sfw_set_path(g._h, C.byref(bad)) == SFW_ERR_INVALID_ARG
        got = g.path()
        assert _same(got[0], good) and got[1] == -0.5  # every refusal leaves the previous setting
    null = SfwPath(None, 3, 0, 1.0)
    assert L.sfw_set_path(g._h, C.byref(null)) == SFW_ERR_INVALID_ARG and _same(g.path()[0], good)
    g.set_path(np.full((SFW_PATH_MAX_POINTS, 2), 1e7), 0.0)  # the largest path, the largest coordinate, weight 0: accepted
    assert g.path()[0].shape == (SFW_PATH_MAX_POINTS, 2)
    # a partial read
    out = np.full((2, 2), 7.0)
    assert L.sfw_get_path(g._h, out.ctypes.data, 2, C.byref(n), None, None) == 0 and n.value == SFW_PATH_MAX_POINTS and np.all(out == 1e7)
    assert L.sfw_get_path(g._h, None, 2, None, None, None) == SFW_ERR_INVALID_ARG
    g.set_path(None)
    assert g.path() is None
    w5 = (1.0, 1.0, 1.0, 1.0, 1.0)
    with pytest.raises(hip_mod.SfwError) as e:
        g.path_term(0, 1)  # before a stage
    assert e.value.status == SFW_ERR_STATE
    # staged without a path, the setter between stage and launch does not reach that launch
    g.stage(RS, LIN, ANG, GOAL)
    g.set_path(good, 2.0)
    g.launch()
    off = np.array(g.fetch()[0])
    assert g.plan_info()["one_launch"] == 1
    for call in (lambda: g.path_term(0, len(off)), lambda: g.rescore_path(w5, (1.0,))):
        with pytest.raises(hip_mod.SfwError) as e:
            call()
        assert e.value.status == SFW_ERR_STATE
    # ... and the other way round: staged with the path, switched off before the launch
    g.stage(RS, LIN, ANG, GOAL)
    g.set_path(None)
    with pytest.raises(hip_mod.SfwError) as e:
        g.path_term(0, len(off))  # staged, not launched yet
    assert e.value.status == SFW_ERR_STATE
    g.launch()
    on = np.array(g.fetch()[0])
    p = g.path_term(0, len(on))
    assert _same(on, P.add(off, p, 2.0)) and (on != off).any()
    for args in ((-1, 1), (0, 0), (0, len(on) + 1), (len(on), 1)):
        with pytest.raises(hip_mod.SfwError) as e:
            g.path_term(*args)
        assert e.value.status == SFW_ERR_INVALID_ARG
    # the largest path through the kernels: 1023 segments, every one of them the same far point but the last two
    far = np.full((SFW_PATH_MAX_POINTS, 2), 50.0)
    far[-2:] = good[:2]
    g.set_path(far, 1.0)
    c, _ = g.score_grid(RS, LIN, ANG, GOAL)
    pts, n_points = g.grid_points_batch(0, len(c), 5)
    want = np.where(np.array(c) == -2.0, -2.0, P.path_term(pts, n_points, far))
    assert _same(g.path_term(0, len(c)), want)
    g.close()


# ---- the C++ host mirror -------------------------------------------------------------------------------------------------------------------
def test_host_mirror_hands_the_window_down(hip_mod):
    """SFWPlanner::setPathTerm: every cycle hands the global plan's points [max(0, wp_index - 1), ...) down, at most max_points; a
    weight of exactly 0 is off.  The pattern of tests/test_host_state_machine.py and of the stop check's host test."""
    from social_force_window_planner_amd import host, synthetic as syn
    from social_force_window_planner_amd._abi import BRANCH_GRID, default_ctrl_params
    host.build()
    scene = syn.make_scene(dataclasses.replace(syn.WORKLOADS["ref5x9"], n_people=0))
    scene.cells[:] = 0
    lin, ang = syn.reference_sampler()
    ctrl = dict(max_trans_acc=0.5, max_rot_acc=1.0)
    plan = np.array([[x, 0.1 * x, 0.0] for x in np.linspace(0.0, 4.0, 17)])
    pose, vel = [0.0, 0.0, 0.0], [0.3, 0.0, 0.0]
    pl = host.HostPlanner(default_ctrl_params(**ctrl), scene)
    pl.update_plan(plan)
    off = pl.find_best_action(pose, vel)
    off_costs = pl.last_costs().copy()
    assert off[2] == BRANCH_GRID and off[0] and pl.path_term() is None  # off by default
    # at the start of the plan the way-point has already moved on past the points within wp_tolerance: one point behind it
    pl.set_path_term(3.0, 5)
    on = pl.find_best_action(pose, vel)
    assert on[2] == BRANCH_GRID
    first = max(0, pl.wp_index - 1)
    xy, w = pl.path_term()
    assert w == 3.0 and _same(xy, plan[first:first + 5, :2]) and len(xy) == 5
    assert (pl.last_costs() != off_costs).any()
    # a plan that begins a metre ahead of the robot: the way-point is point 0, and so is the window's first point
    ahead = plan + np.array([1.0, 0.0, 0.0])
    pa = host.HostPlanner(default_ctrl_params(**ctrl), scene)
    pa.update_plan(ahead)
    pa.set_path_term(3.0, 5)
    assert pa.find_best_action(pose, vel)[2] == BRANCH_GRID and pa.wp_index == 0
    xy, w = pa.path_term()
    assert w == 3.0 and _same(xy, ahead[:5, :2])
    pa.close()
    # further along (a new plan makes the planner look for its way-point again): the window begins one point BEHIND it
    pose2 = [1.6, 0.16, 0.1]
    pl.update_plan(plan)
    on2 = pl.find_best_action(pose2, vel)
    i = pl.wp_index
    assert on2[2] == BRANCH_GRID and i >= 2
    xy, w = pl.path_term()
    assert w == 3.0 and _same(xy, plan[i - 1:i + 4, :2]) and len(xy) == 5
    on2_costs = pl.last_costs().copy()
    # ... and the cycle is what a handle given that window itself returns
    g = hip_mod.HipScorer(default_params(sim_time=1.0, sim_granularity=0.025))
    g.load_scene(scene)
    rs = tuple(float(np.float32(v)) for v in (*pose2, *vel))
    goal = (0.5, 0.0, 1.0, float(plan[i][0]), float(plan[i][1]))
    plain, _ = g.score_grid(rs, lin, ang, goal)
    g.set_path(xy, 3.0)
    costs, best = g.score_grid(rs, lin, ang, goal)
    p = g.path_term(0, len(costs))
    assert _same(on2_costs, costs) and _same(on2_costs, P.add(plain, p, 3.0))
    assert on2[1].tolist() == [best["vx"], 0.0, best["vtheta"]]
    g.close()
    # the default max_points: to the end of the plan; a cap beyond SFW_PATH_MAX_POINTS is clamped
    for cap in (None, 10 ** 6):
        pl.set_path_term(-1.5) if cap is None else pl.set_path_term(-1.5, cap)
        pl.find_best_action(pose2, vel)
        xy, w = pl.path_term()
        assert w == -1.5 and _same(xy, plan[pl.wp_index - 1:, :2])
    pl.set_path_term(2.0, 0)  # ... and one below 1 as well: one point
    pl.find_best_action(pose2, vel)
    assert _same(pl.path_term()[0], plan[pl.wp_index - 1:pl.wp_index, :2])
    # a weight of exactly 0: off, and the cycle is the path-off cycle bit for bit
    pl.set_path_term(0.0)
    pl.update_plan(plan)
    again = pl.find_best_action(pose, vel)
    assert pl.path_term() is None and again[0] == off[0] and again[2] == off[2] and _same(again[1], off[1])
    assert _same(pl.last_costs(), off_costs)
    pl.close()
