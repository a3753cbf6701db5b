"""The footprint clearance map on the device (sfw_set_footprint_clearance): the map the two kernels build against the numpy
window rule, and every launch path with the map on against the same launch with it off — bit for bit in costs, sentinels,
selection, captured terms, Trajectory points and point counts — and against the oracle at 1e-9.

The scenes: a 40 x 30 map (non-square) with the robot in the middle of cell (22, 15), five pedestrians, and ONE cost cell in the
corner of the robot's window at per-axis offset r_c - 1, r_c (inside the window: the start pose is not clear and walks) or
r_c + 1 (outside: the start pose is clear).  The samples drive towards the right border: their later poses' windows, then their
footprints, leave the map.  SFW_CLEAR_MIN_POSES=0 lets every stage build the map (the default builds from 368 640 poses on);
K1b as a kernel of its own runs for grids of more than 2048 samples (the `wide` paths: what reads the map), the small grids run
the fused K1 and the one-launch cycle kernel, which do not read it and must not care."""
import dataclasses

import numpy as np
import pytest

import clearance_reference as CR
import costmap_reference as R
from sfw_test_util import _same
from social_force_window_planner_amd import synthetic as syn
from social_force_window_planner_amd._abi import default_params

pytestmark = pytest.mark.gpu

SX, SY, CX, CY = 40, 30, 22, 15
BIG_BOX = [[0.5, 0.3], [-0.5, 0.3], [-0.5, -0.3], [0.5, -0.3]]
FOOTPRINTS = {"polygon16": R.polygon16(), "box": np.array(R.BOX), "k2": np.array(CR.K2_FOOTPRINT), "big_box": np.array(BIG_BOX)}


def _scene(cells, fp, res=0.05):
    """the reference's 5 x 9 scene on a 40 x 30 map whose cell (CX, CY) has the robot (0, 0) at its centre"""
    base = syn.make_scene("ref5x9")
    return dataclasses.replace(base, cells=np.ascontiguousarray(cells, dtype=np.uint8), origin_x=-(CX + 0.5) * res, origin_y=-(CY + 0.5) * res,
                               resolution=res, footprint=np.asarray(fp, dtype=np.float64).reshape(-1, 2))


def _cells(*marks):
    cells = np.zeros((SY, SX), dtype=np.uint8)
    for x, y, v in marks:
        cells[y, x] = v
    return cells


def _corner(fp, res, off):
    """one cost-1 cell at per-axis offset r_c + off from the robot's cell"""
    r = CR.half_width(fp, res)
    return _cells((CX + r + off, CY + r + off, 1))


def _params(S=40):
    return default_params(sim_time=1.0, sim_granularity=1.0 / S)


def _scorer(hip_mod, monkeypatch, S=40, min_poses="0"):
    if min_poses is None:
        monkeypatch.delenv("SFW_CLEAR_MIN_POSES", raising=False)
    else:
        monkeypatch.setenv("SFW_CLEAR_MIN_POSES", min_poses)
    monkeypatch.setenv("SFW_CYCLE_FUSED", "1")
    g = hip_mod.HipScorer(_params(S))
    g.set_terms_capture(True)
    return g


# ---- the launch paths ----------------------------------------------------------------------------------------------------------
WIDE = 48  # 48 x 48 = 2304 samples: more than the fused K1 takes
PATHS = ["grid5x9", "grid8x6_s8", "grid_small", "grid_wide", "list", "list_wide", "sequence", "sequence_wide"]


def _steps(path):
    return 8 if path == "grid8x6_s8" else 40


def _commands(path, scene):
    if path in ("grid5x9", "grid_small"):
        return scene.linvels, scene.angvels
    if path == "grid8x6_s8":
        return syn.generalised_sampler(8, 6)
    if path == "grid_wide":
        return syn.generalised_sampler(WIDE, WIDE)
    if path == "grid_96":
        return syn.generalised_sampler(96, 96)
    n = WIDE * WIDE if path.endswith("wide") else 45
    rng = np.random.default_rng(5)
    return rng.uniform(0.0, 0.7, n), rng.uniform(-0.5, 0.5, n)


def _launch(g, monkeypatch, path, scene, on):
    """one blocking call of `scene` through `path` with the switch on or off: everything a caller can read back"""
    monkeypatch.setenv("SFW_CYCLE_FUSED", "0" if path == "grid_small" else "1")
    S = _steps(path)
    g.set_params(_params(S))
    g.set_footprint_clearance(on)
    g.load_scene(scene)
    a, b = _commands(path, scene)
    if path.startswith("grid"):
        costs, best = g.score_grid(scene.robot_state, a, b, scene.goal_args)
    elif path.startswith("list"):
        costs, best = g.score_samples(scene.robot_state, a, b, scene.goal_args, vy=0.2 * b)
    else:
        costs, best = g.score_sequences(scene.robot_state, np.stack([a, a[::-1]]), np.stack([b, b[::-1]]), (0, 11), scene.goal_args,
                                        vy=np.stack([0.2 * b, 0.1 * a]))
    T = len(costs)
    info = g.plan_info()
    assert info["samples"] == T and (info["one_launch"] == 1) == (path in ("grid5x9", "grid8x6_s8", "list", "sequence")), info
    built, r = g.footprint_clearance_info()
    pts, n = g.grid_points_batch(0, T, S)
    return R.NS(costs=np.array(costs), best=best, terms=g.cost_terms().copy(), pts=pts, n=n, built=built, r=r)


def _assert_identical(x, y, what):
    assert _same(x.costs, y.costs), what
    assert x.best == y.best, (what, x.best, y.best)
    assert _same(x.terms, y.terms) and _same(x.pts, y.pts) and np.array_equal(x.n, y.n), what


def _oracle_costs(oracle_mod, path, scene):
    a, b = _commands(path, scene)
    o = oracle_mod.OracleScorer(_params(_steps(path)))
    o.load_scene(scene)
    if path.startswith("grid"):
        oc, _ = o.score_grid(scene.robot_state, a, b, scene.goal_args, n_threads=8)
        return oc
    return np.array([o.score_one(scene.robot_state, a[t], 0.2 * b[t], b[t], scene.goal_args)[0] for t in range(len(a))])


def _assert_oracle(costs, oc, what):
    assert np.array_equal(oc < 0, costs < 0), what
    v = oc > 0
    assert np.all(np.abs(costs[v] - oc[v]) <= 1e-9 * np.abs(oc[v])), (what, float(np.max(np.abs(costs[v] - oc[v]) / np.abs(oc[v]))))


# ---- the map itself --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname,res", [("polygon16", 0.05), ("box", 0.05), ("k2", 0.05), ("polygon16", 0.03)])
def test_device_map_is_the_window_rule(hip_mod, monkeypatch, fname, res):
    """the corner cell at offset r_c - 1, r_c, r_c + 1: the robot's cell is clear for the last alone; the whole map is numpy's"""
    fp = FOOTPRINTS[fname]
    r = CR.half_width(fp, res)
    assert CY - r - 1 >= 0 and CY + r + 1 < SY  # the three corners are on the map
    g = _scorer(hip_mod, monkeypatch, 8)
    lin, ang = syn.generalised_sampler(8, 6)
    seen = []
    for off in (-1, 0, 1):
        scene = _scene(_corner(fp, res, off), fp, res)
        g.load_scene(scene)
        g.stage(scene.robot_state, lin, ang, scene.goal_args)
        assert g.footprint_clearance_info() == (True, r)
        got = g.footprint_clearance_map(SY, SX)
        assert np.array_equal(got, CR.clearance_map(scene.cells, r)), (fname, res, off)
        seen.append(int(got[CY, CX]))
        assert got[:r].sum() == 0 and got[:, :r].sum() == 0 and got[SY - r:].sum() == 0 and got[:, SX - r:].sum() == 0  # windows that leave the map
    assert seen == [0, 0, 1]
    g.close()


def test_maps_with_many_cells_and_lone_rows(hip_mod, monkeypatch):
    """random sparse maps, a one-row strip and a one-column strip: the device's map is numpy's"""
    fp = FOOTPRINTS["k2"]
    r = CR.half_width(fp, 0.05)
    g = _scorer(hip_mod, monkeypatch, 8)
    rng = np.random.default_rng(3)
    base = _scene(_cells(), fp)
    for sy, sx in ((30, 40), (1, 300), (300, 1), (257, 259), (13, 2 * r + 1)):
        cells = (rng.uniform(size=(sy, sx)) < 0.002).astype(np.uint8) * rng.integers(1, 256, (sy, sx)).astype(np.uint8)
        scene = dataclasses.replace(base, cells=cells)
        g.load_scene(scene)
        g.stage(scene.robot_state, base.linvels, base.angvels, scene.goal_args)
        assert g.footprint_clearance_info() == (True, r)
        assert np.array_equal(g.footprint_clearance_map(sy, sx), CR.clearance_map(cells, r)), (sy, sx)
    g.close()


# ---- on against off, and the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_on_off_identical_and_oracle(hip_mod, oracle_mod, monkeypatch, path):
    fp = FOOTPRINTS["polygon16"]
    g = _scorer(hip_mod, monkeypatch)
    # the three corners, and a lethal cell ahead of the robot that the faster samples' footprints reach
    scenes = [_scene(_corner(fp, 0.05, off), fp) for off in (-1, 0, 1)] + [_scene(_cells((CX + 12, CY + 1, 254), (CX + 3, CY - 9, 90)), fp)]
    for k, scene in enumerate(scenes):
        on = _launch(g, monkeypatch, path, scene, True)
        off = _launch(g, monkeypatch, path, scene, False)
        assert on.built and on.r == CR.half_width(fp, 0.05) and not off.built
        _assert_identical(on, off, (path, k))
        assert np.any(on.costs == -1.0) and np.any(on.costs >= 0.0), (path, k)  # some samples leave the map, some are scored
        if path.startswith("grid") or path == "list":
            _assert_oracle(on.costs, _oracle_costs(oracle_mod, path, scene), (path, k))
    g.close()


def test_k2_footprint(hip_mod, oracle_mod, monkeypatch):
    """fewer than three vertices: the centre cell alone is read, and a clear one reads 0"""
    fp = FOOTPRINTS["k2"]
    g = _scorer(hip_mod, monkeypatch)
    for scene in (_scene(_corner(fp, 0.05, 1), fp), _scene(_cells((CX + 4, CY, 120), (CX + 9, CY + 1, 254), (CX + 9, CY, 253)), fp)):
        on = _launch(g, monkeypatch, "grid_wide", scene, True)
        off = _launch(g, monkeypatch, "grid_wide", scene, False)
        assert on.built and on.r == 6
        _assert_identical(on, off, "k2")
        _assert_oracle(on.costs, _oracle_costs(oracle_mod, "grid_wide", scene), "k2")
    g.close()


def test_footprint_too_large_for_a_map(hip_mod, monkeypatch):
    """a window of more than 129 cells: no map is built, every pose walks"""
    a = np.arange(8) * (2 * np.pi / 8)
    fp = np.stack([3.3 * np.cos(a), 3.3 * np.sin(a)], axis=1)
    assert CR.half_width(fp, 0.05) is None
    g = _scorer(hip_mod, monkeypatch)
    big = dataclasses.replace(_scene(np.zeros((300, 300), dtype=np.uint8), fp), origin_x=-7.525, origin_y=-7.525)
    on = _launch(g, monkeypatch, "grid_wide", big, True)
    off = _launch(g, monkeypatch, "grid_wide", big, False)
    assert (on.built, on.r) == (False, -1)
    _assert_identical(on, off, "large footprint")
    assert np.any(on.costs >= 0.0)
    g.close()


# ---- what makes the map stale ----------------------------------------------------------------------------------------------------
def _all_rejected(out):
    return bool(np.all(out.costs < 0) and np.all(out.n == 0))


@pytest.mark.parametrize("path", ["grid_wide", "list_wide"])
def test_changed_map_footprint_and_resolution_are_seen(hip_mod, monkeypatch, path):
    """One handle, the map on.  Every change below turns the start pose from clear to blocked by a lethal cell OUTSIDE the window
    the map was last built for, or back: a map that was not rebuilt would score what the launch before scored."""
    poly, big = FOOTPRINTS["polygon16"], FOOTPRINTS["big_box"]
    free, wall = _cells(), _cells((CX + 10, CY, 254))  # ten cells ahead: beyond polygon16's r_c = 8, on big_box's front edge
    g = _scorer(hip_mod, monkeypatch)
    fresh = _scorer(hip_mod, monkeypatch)

    def both(scene, what):
        on = _launch(g, monkeypatch, path, scene, True)
        assert on.built, what
        _assert_identical(on, _launch(fresh, monkeypatch, path, scene, False), what)
        return on

    # the cells: clear -> blocked -> clear
    a = both(_scene(free, big), "free")
    assert not _all_rejected(a)
    assert _all_rejected(both(_scene(wall, big), "wall"))
    assert _same(both(_scene(free, big), "free again").costs, a.costs)
    # the footprint: polygon16 passes the wall's cell at the start (the cell is outside its window only if the map is its own)
    p = both(_scene(wall, poly), "polygon16 by the wall")
    assert not _all_rejected(p) and p.r == 8
    q = both(_scene(wall, big), "big box by the wall")
    assert _all_rejected(q) and q.r == 13
    assert _same(both(_scene(wall, poly), "polygon16 again").costs, p.costs)
    # the resolution: at 0.034 m the same cells put the wall's cell under polygon16's front vertex (0.35 m = 10.3 cells ahead)
    h = both(_scene(wall, poly, 0.034), "a finer resolution")
    assert _all_rejected(h) and h.r == 12
    assert _same(both(_scene(wall, poly), "0.05 again").costs, p.costs)
    # the geometry: the same bytes as a 30 x 40 map
    t = dataclasses.replace(_scene(wall, poly), cells=np.ascontiguousarray(wall.reshape(SX, SY)))
    both(t, "turned")
    assert _same(both(_scene(wall, poly), "turned back").costs, p.costs)
    g.close()
    fresh.close()


# ---- when the map is built ---------------------------------------------------------------------------------------------------------
def test_small_grids_do_not_build_and_the_switch_turns_it_off(hip_mod, monkeypatch):
    fp = FOOTPRINTS["polygon16"]
    scene = _scene(_corner(fp, 0.05, 1), fp)
    g = _scorer(hip_mod, monkeypatch, min_poses=None)  # the default threshold
    assert not _launch(g, monkeypatch, "grid5x9", scene, True).built  # 1800 poses
    assert not _launch(g, monkeypatch, "grid8x6_s8", scene, True).built
    assert not _launch(g, monkeypatch, "grid_wide", scene, True).built  # 2304 x 40 = 92 160 poses
    wide = _launch(g, monkeypatch, "grid_96", scene, True)  # 9216 x 40 = 368 640 poses: the threshold
    assert wide.built and wide.r == 8
    assert _launch(g, monkeypatch, "grid5x9", scene, True).built  # the map is there now and describes this costmap
    assert not _launch(g, monkeypatch, "grid_96", scene, False).built
    g.set_params(_params(8))
    changed = dataclasses.replace(scene, cells=_corner(fp, 0.05, 0))
    assert not _launch(g, monkeypatch, "grid8x6_s8", changed, True).built  # a changed map, 384 poses: not rebuilt
    g.close()
