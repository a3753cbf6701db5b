"""sfw_set_stop_check on the device: the braking tail behind the rollout, against tests/stop_reference.py.

Every comparison is an integer decision or a fixed IEEE sequence: sentinels, tail lengths, first illegal poses, velocities,
headings and — at heading 0 — poses are asserted BIT FOR BIT.  Where a pose goes through the device's sincos it is held to
rollout_reference.pose_bound at SINCOS_ULP_DEVICE, and the footprint verdict is taken on the device's OWN tail poses
(stop_points), as tests/test_costmap_edges_gpu.py does for the rollout's.

Paths (plan_info() says which one ran; with the check on no path is the one-launch kernel):
    small        sfw_rollout_small_kernel, then the tail            k1abc      K1a (teams) + K1b + K1c, then the tail: > 2048 samples
    k1abc_thr    the same with SFW_K1A_THREADS=1                    list_small, list_k1abc   the LIST instantiations
    sequence     two knots, S + 1 steps: the SEQ instantiation"""
import math

import numpy as np
import pytest

import costmap_reference as CR
import rollout_reference as RR
import stop_reference as SR
from sfw_test_util import _bits, _np_best, _same
from social_force_window_planner_amd._abi import (SFW_ERR_INVALID_ARG, SFW_STOP_MAX_STEPS, SFW_STOP_NONE, SFW_STOP_NOT_RUN, SFW_STOP_UNFINISHED, SfwAgent,
                                                  SfwStopCheck, default_params)

pytestmark = pytest.mark.gpu

PATHS = ["small", "k1abc", "k1abc_thr", "list_small", "list_k1abc", "sequence"]
WIDE = 2049  # more samples than the fused small-grid K1 takes


def _params(S, dt):
    return default_params(sim_time=S * dt, sim_granularity=dt)


def _no_agents():
    return (SfwAgent * 0)()


def _env(monkeypatch, path):
    monkeypatch.setenv("SFW_CYCLE_FUSED", "0")  # (the check-off runs take the same kernels as the check-on ones)
    monkeypatch.setenv("SFW_K1A_THREADS", "1" if path == "k1abc_thr" else "0")


def _commands(path, cmds):
    """the (vx, vth) list of a launch through `path` and, per sample, its index into the n base commands"""
    n = len(cmds)
    k = -(-WIDE // n) if path in ("k1abc", "k1abc_thr", "list_k1abc") else 1
    idx = np.arange(k * n) % n
    return idx


def _score(g, path, case, S):
    """one launch of a wall case: (costs, best, idx, vx, vth)"""
    n = len(case.lin) * len(case.ang)
    cmds = RR.product(case.lin, case.ang)
    idx = _commands(path, cmds)
    if path in ("small", "k1abc", "k1abc_thr"):
        lin = np.tile(case.lin, len(idx) // n)
        costs, best = g.score_grid(case.rs, lin, case.ang, case.goal)
    elif path == "sequence":
        vx, vth = cmds[:, 0], cmds[:, 2]
        costs, best = g.score_sequences(case.rs, np.stack([vx, vx[::-1]]), np.stack([vth, vth[::-1]]), (0, 1), case.goal)
    else:
        costs, best = g.score_samples(case.rs, cmds[idx, 0], cmds[idx, 2], case.goal)
    info = g.plan_info()
    assert info["one_launch"] == 0 and info["samples"] == len(idx) and info["chunks"] == 1, info
    assert (info["samples"] > 2048) == (path in ("k1abc", "k1abc_thr", "list_k1abc")), info
    return np.array(costs), best, idx, cmds[idx, 0], cmds[idx, 2]


def _load(g, case, S):
    g.set_params(_params(S, case.dt))
    g.set_costmap(case.map.cells, case.map.origin_x, case.map.origin_y, case.map.resolution)
    g.set_footprint(case.footprint)
    g.set_agents(_no_agents())
    g.set_terms_capture(True)


# ---- 1. wall ahead, exact: the test that fails without the feature --------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_wall_ahead_exact(hip_mod, monkeypatch, path):
    _env(monkeypatch, path)
    g = hip_mod.HipScorer(_params(2, SR.WALL_DT))
    seen = set()
    for case in SR.wall_cases():
        ref = SR.wall_reference(case, sequence=path == "sequence")
        S = ref.S
        _load(g, case, S)
        g.set_stop_check(None)
        off, off_best, idx, vx, vth = _score(g, path, case, S)
        off_terms = g.cost_terms()
        scored = ~ref.skipped[idx] if path in ("small", "k1abc", "k1abc_thr") else np.ones(len(idx), dtype=bool)
        assert np.all(off[scored] >= 0.0), case.name  # the rollout alone rejects nothing
        with pytest.raises(hip_mod.SfwError):
            g.stop_info(0, len(idx))  # the staged grid has the check off

        g.set_stop_check((*case.dec, case.max_steps))
        on, on_best, _, _, _ = _score(g, path, case, S)
        on_terms = g.cost_terms()
        steps, hit = g.stop_info(0, len(idx))
        want_rej = np.array([w[0] for w in ref.want])[idx] & scored
        want_hit = np.array([w[1] for w in ref.want])[idx]
        want_hit = np.where(scored, want_hit, SFW_STOP_NOT_RUN)
        want_steps = np.where(scored, ref.steps[idx], 0)
        assert np.array_equal(on == -1.0, want_rej), (case.name, on, want_rej)
        assert np.array_equal(steps, want_steps) and np.array_equal(hit, want_hit), (case.name, steps, want_steps, hit, want_hit)
        assert np.all(on_terms[want_rej] == -1.0)
        keep = ~want_rej
        assert _same(on[keep], off[keep]) and _same(on_terms[keep], off_terms[keep]), case.name
        # the tail poses, bit for bit against the exact layer
        cap = max(int(ref.tail.vx.shape[0]), 1)
        pts, n_steps = g.stop_points(0, len(idx), cap)
        assert np.array_equal(n_steps, want_steps), case.name
        for j in range(ref.tail.vx.shape[0]):
            live = j < want_steps
            assert RR.same_but_zero_sign(pts[live, j], ref.poses[j][idx][live]), (case.name, j)
        # the selection is the selection over the survivors
        nb = _np_best(on, vx, None, vth)
        assert on_best["index"] == nb["index"] and (nb["index"] < 0 or on_best["cost"] == nb["cost"]), (case.name, on_best, nb)
        assert nb["index"] < 0 or not want_rej[nb["index"]]
        seen |= {int(h) if h < 0 else "hit" for h in hit[scored]}
        # ... and switching the check off restores the check-off result bit for bit
        g.set_stop_check(None)
        again, again_best, _, _, _ = _score(g, path, case, S)
        assert _same(again, off) and _same(g.cost_terms(), off_terms) and again_best == off_best, case.name
    assert {SFW_STOP_NONE, SFW_STOP_UNFINISHED, "hit"} <= seen
    g.close()


# ---- 2. random headings ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname,fname,seed,holonomic", SR.RANDOM_CASES)
def test_random_headings(hip_mod, monkeypatch, gname, fname, seed, holonomic):
    _env(monkeypatch, "list_small")
    case = SR.random_case(gname, fname, seed, holonomic)
    ex, tl, hp, bx, by = SR.random_reference(case)
    S, m = case.S, tl.vx.shape[0]
    assert not tl.unfinished.any() and tl.steps.min() >= 1 and m >= 4
    g = hip_mod.HipScorer(_params(S, case.dt))
    g.set_costmap(case.map.cells, case.map.origin_x, case.map.origin_y, case.map.resolution)
    g.set_footprint(case.footprint)
    g.set_agents(_no_agents())
    goal = (*case.acc, case.rs[0], case.rs[1])
    g.set_stop_check(None)
    off, _ = g.score_samples(case.rs, case.cmds[:, 0], case.cmds[:, 2], goal, vy=case.cmds[:, 1])
    g.set_stop_check((*case.dec, case.max_steps))
    on, _ = g.score_samples(case.rs, case.cmds[:, 0], case.cmds[:, 2], goal, vy=case.cmds[:, 1])
    n = len(on)
    steps, hit = g.stop_info(0, n)
    pts, n_steps = g.stop_points(0, n, m)
    ran = off >= 0.0
    assert ran.sum() >= n // 2  # (the map leaves most rollouts legal)
    assert np.array_equal(steps[ran], tl.steps[ran]) and np.array_equal(n_steps, steps)  # the tail's length is exact
    assert np.all(steps[~ran] == 0) and np.all(hit[~ran] == SFW_STOP_NOT_RUN)
    tally, worst = {}, 0.0
    for j in range(m):
        live = ran & (j < steps)
        # headings bit for bit.  (stop_points hands out no velocities: the angular one is held through these sums, vx and vy
        # through the exact tail length above — one ulp in either moves the step at which both reach 0 only by chance, so they
        # are held to pose_bound below as well, not bit for bit on their own)
        assert _same(pts[live, j, 2], tl.th[j + 1][live]), j
        ex_x, ex_y = hp.x[S + j + 1], hp.y[S + j + 1]
        dx = np.abs((pts[:, j, 0] - ex_x) - hp.x_lo[S + j + 1])
        dy = np.abs((pts[:, j, 1] - ex_y) - hp.y_lo[S + j + 1])
        assert np.all(dx[live] <= bx[S + j + 1][live]) and np.all(dy[live] <= by[S + j + 1][live]), j
        worst = max(worst, float(np.max(np.concatenate([dx[live] / bx[S + j + 1][live], dy[live] / by[S + j + 1][live], [0.0]]))))
    # the verdict on the device's own tail poses
    want = SR.verdict(case.map, case.footprint, pts, np.where(ran, steps, 0), np.zeros(n, dtype=bool), tally)
    checked = 0
    for t in np.flatnonzero(ran):
        if want[t] is None:
            continue
        checked += 1
        assert (bool(on[t] == -1.0), int(hit[t])) == want[t], (t, on[t], hit[t], want[t])
        if not want[t][0]:
            assert _same(on[t], off[t])
    print(f"{case.name}: {tally['left_out']} of {tally['poses']} tail poses left out, {checked} samples checked, worst pose error "
          f"{worst:.3f} of its bound, {int((on[ran] == -1.0).sum())} rejected")
    assert tally["left_out"] <= 0.01 * tally["poses"] and tally["poses"] >= 300, tally
    assert (on[ran] == -1.0).any() and (on[ran] >= 0.0).any()
    g.close()


# ---- 3. equality across organisations --------------------------------------------------------------------------------------------------
def _full(g, n, cap):
    steps, hit = g.stop_info(0, n)
    pts, ns = g.stop_points(0, n, cap)
    return steps, hit, pts, ns


def _assert_equal_runs(a, b, what):
    assert _same(a[0], b[0]), what
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(_bits(x) if x.dtype == np.float64 else x, _bits(y) if y.dtype == np.float64 else y), what


@pytest.fixture(scope="module")
def org_scene():
    geo = CR.geometry("wide_120x80_r0.05")
    x0, y0 = CR.mid_cell(geo.origin_x, geo.resolution, geo.size_x), CR.mid_cell(geo.origin_y, geo.resolution, geo.size_y)
    m = CR.random_map(geo, 11, (x0, y0), clear_radius=1.0)
    # ... with a lethal ring 1 m around the start: beyond every rollout (0.4 m and the box's 0.5 m), inside the longer braking paths
    my, mx = np.mgrid[0:geo.size_y, 0:geo.size_x]
    d = np.hypot(geo.origin_x + (mx + 0.5) * geo.resolution - x0, geo.origin_y + (my + 0.5) * geo.resolution - y0)
    cells = m.cells.copy()
    cells[(d > 1.0) & (d < 1.1)] = 254
    m = CR.make_map(cells, geo.origin_x, geo.origin_y, geo.resolution)
    lin = np.linspace(0.05, 0.65, 64)
    ang = np.linspace(-0.5, 0.5, 33)
    return CR.NS(map=m, rs=(x0, y0, 0.7, 0.3, 0.0, 0.2), lin=lin, ang=ang, goal=(1.0, 0.7, 1.3, x0 + 1.0, y0), S=20, dt=0.03125,
                 check=(0.6, 0.6, 1.0, 64), cap=40)


def _org_run(hip_mod, sc, kind, clearance=True, lin=None, ang=None):
    g = hip_mod.HipScorer(_params(sc.S, sc.dt))
    g.set_costmap(sc.map.cells, sc.map.origin_x, sc.map.origin_y, sc.map.resolution)
    g.set_footprint(CR.FOOTPRINTS["box"])
    g.set_agents(_no_agents())
    g.set_footprint_clearance(clearance)
    g.set_stop_check(sc.check)
    lin = sc.lin if lin is None else lin
    ang = sc.ang if ang is None else ang
    cmds = RR.product(lin, ang)
    if kind == "grid":
        costs, _ = g.score_grid(sc.rs, lin, ang, sc.goal)
    elif kind == "list":
        costs, _ = g.score_samples(sc.rs, cmds[:, 0], cmds[:, 2], sc.goal)
    else:  # a one-knot sequence
        costs, _ = g.score_sequences(sc.rs, cmds[None, :, 0], cmds[None, :, 2], (0,), sc.goal)
    info = g.plan_info()
    out = (np.array(costs), _full(g, len(costs), sc.cap), info, cmds)
    g.close()
    return out


def test_equal_across_organisations(hip_mod, monkeypatch, org_scene):
    sc = org_scene
    monkeypatch.setenv("SFW_CYCLE_FUSED", "0")
    monkeypatch.setenv("SFW_CLEAR_MIN_POSES", "0")  # (every stage builds the clearance map)
    base = _org_run(hip_mod, sc, "grid")
    T = len(base[0])
    assert T > 2048 and base[2]["chunks"] == 1 and base[2]["one_launch"] == 0
    assert (base[0] == -1.0).any() and (base[0] >= 0).any() and (base[1][1] >= 0).any() and (base[1][1] == SFW_STOP_NONE).any()
    # grid against list against one-knot sequence (all k1abc)
    for kind in ("list", "seq"):
        _assert_equal_runs(base, _org_run(hip_mod, sc, kind), kind)
    # team against thread K1a
    monkeypatch.setenv("SFW_K1A_THREADS", "1")
    _assert_equal_runs(base, _org_run(hip_mod, sc, "grid"), "thread K1a")
    monkeypatch.setenv("SFW_K1A_THREADS", "0")
    # clearance map on against off
    _assert_equal_runs(base, _org_run(hip_mod, sc, "grid", clearance=False), "clearance off")
    # two or more chunks against one (1 MB of tables: 1024-sample chunks, the floor)
    monkeypatch.setenv("SFW_TABLE_BUDGET_MB", "1")
    chunked = _org_run(hip_mod, sc, "grid")
    assert chunked[2]["chunks"] >= 2, chunked[2]
    _assert_equal_runs(base, chunked, "chunks")
    monkeypatch.delenv("SFW_TABLE_BUDGET_MB")
    # ... with chunks too large for the fused small K1 (a 64 x 99 grid under 4 MB of tables: chunks of ~2 770 samples), so that the
    # tail runs behind K1a + K1b + K1c at chunk_begin != 0
    ang99 = np.linspace(-0.5, 0.5, 99)
    wide = _org_run(hip_mod, sc, "grid", ang=ang99)
    assert wide[2]["chunks"] == 1 and wide[2]["samples"] == 64 * 99
    monkeypatch.setenv("SFW_TABLE_BUDGET_MB", "4")
    wide_chunked = _org_run(hip_mod, sc, "grid", ang=ang99)
    monkeypatch.delenv("SFW_TABLE_BUDGET_MB")
    info = wide_chunked[2]
    assert info["chunks"] >= 2 and info["samples"] / info["chunks"] > 2048, info
    _assert_equal_runs(wide, wide_chunked, "large chunks")
    # a tail table shorter than the tails (3 rows, then none): the steps beyond it are checked by the thread that walks the tail
    for rows_max in ("3", "0"):
        monkeypatch.setenv("SFW_STOP_TABLE_ROWS", rows_max)
        _assert_equal_runs(base, _org_run(hip_mod, sc, "grid"), "table rows " + rows_max)
    monkeypatch.delenv("SFW_STOP_TABLE_ROWS")
    assert base[1][0].max() > 3
    # small against k1abc: the first 31 rows of the grid (2046 samples: the fused K1) equal the same rows of the wide launch
    rows = 2046 // len(sc.ang)
    small = _org_run(hip_mod, sc, "grid", lin=sc.lin[:rows])
    n = rows * len(sc.ang)
    assert small[2]["samples"] == n <= 2048
    assert _same(small[0], base[0][:n])
    for x, y in zip(small[1], base[1]):
        assert np.array_equal(_bits(x) if x.dtype == np.float64 else x, _bits(y[:n]) if y.dtype == np.float64 else y[:n])
    small_list = _org_run(hip_mod, sc, "list", lin=sc.lin[:rows])
    _assert_equal_runs(small, small_list, "small list")


# ---- 4. with people --------------------------------------------------------------------------------------------------------------------
def _people_scene(n_people, contact=False):
    """a one-second scene with people and a lethal ring 1.3 m around the robot: beyond every rollout (0.7 m and the footprint's
    0.35 m at most), inside the braking path of the faster samples.  contact: person 1 stands 0.9 m ahead of the robot, where
    the fastest samples (0.7 m/s, every angular target) touch it at step 28 or 29 of 32 — samples whose rollout poses are all
    legal, whose braking path hits the ring, and whose Trajectory ends at the contact"""
    import ctypes as C
    import dataclasses

    from sfw_test_util import _workload
    from social_force_window_planner_amd import synthetic as syn
    base = syn.make_scene(_workload(n_people, 31, 0))
    sy, sx = base.cells.shape
    my, mx = np.mgrid[0:sy, 0:sx]
    d = np.hypot(base.origin_x + (mx + 0.5) * base.resolution - base.robot_state[0],
                 base.origin_y + (my + 0.5) * base.resolution - base.robot_state[1])
    cells = base.cells.copy()
    cells[(d > 1.3) & (d < 1.4)] = 254
    agents = base.agents
    if contact:
        agents = (type(base.agents[0]) * len(base.agents))()
        for a in range(len(base.agents)):
            C.memmove(C.byref(agents[a]), C.byref(base.agents[a]), C.sizeof(agents[a]))
        p = agents[1]
        p.x, p.y, p.vx, p.vy, p.has_goal, p.desired_velocity = base.robot_state[0] + 0.9, base.robot_state[1], 0.0, 0.0, 0, 0.0
    return dataclasses.replace(base, cells=cells, agents=agents)


@pytest.mark.parametrize("n_people", [5, 20])
def test_with_people_small_grid(hip_mod, monkeypatch, n_people):
    """the smallest crowds that take the register and the flat form: stop-rejected samples read -1, every other sample is
    bit-identical to the check-off run; a sample both stop-rejected and in pedestrian contact reads -1 and keeps the contact's
    point count; score_one and score_one_crowd equal the grid's entry"""
    from sfw_test_util import _params as _scene_params
    monkeypatch.setenv("SFW_CYCLE_FUSED", "1")
    scene = _people_scene(n_people, contact=True)
    g = hip_mod.HipScorer(_scene_params())
    g.load_scene(scene)
    g.set_terms_capture(True)
    g.set_points_capture(True)
    lin, ang = np.linspace(0.0, 0.7, 7), np.linspace(-0.5, 0.5, 9)
    off, _ = g.score_grid(scene.robot_state, lin, ang, scene.goal_args)
    off_terms = g.cost_terms()
    T = len(off)
    S = 32
    off_pts, off_n = g.grid_points_batch(0, T, S)
    check = (0.25, 0.25, 1.0, 256)  # a long braking path: some samples run into what lies beyond their rollout
    g.set_stop_check(check)
    on, best = g.score_grid(scene.robot_state, lin, ang, scene.goal_args)
    assert g.plan_info()["one_launch"] == 0
    on_terms = g.cost_terms()
    steps, hit = g.stop_info(0, T)
    on_pts, on_n = g.grid_points_batch(0, T, S)
    stopped = (hit >= 0) | (hit == SFW_STOP_UNFINISHED)
    assert stopped.any() and (~stopped & (off >= 0)).any(), (hit, off)
    assert np.all(on[stopped] == -1.0) and np.all(on_terms[stopped] == -1.0)
    assert _same(on[~stopped], off[~stopped]) and _same(on_terms[~stopped], off_terms[~stopped])
    # (the tail runs for every sample that is VALID behind the costmap scan: a pedestrian contact is found later, by K2)
    assert np.all(hit[off == -2.0] == SFW_STOP_NOT_RUN) and np.all(hit[off != -2.0] != SFW_STOP_NOT_RUN)
    # the Trajectory keeps its points: S for a stop-rejected sample, the contact's count for one also in contact (no rollout
    # pose is illegal in this scene, so a check-off count below S IS a contact: its step + 1)
    assert np.array_equal(on_n, off_n) and _same(on_pts, off_pts)
    scored = off != -2.0
    both = (hit >= 0) & (off_n < S) & scored
    assert both.sum() >= 3 and np.all(off[both] == -1.0) and np.all(off_n[both] >= 1), (hit, off_n)
    assert np.all(on[both] == -1.0) and np.all(on_terms[both] == -1.0) and np.array_equal(on_n[both], off_n[both])
    assert (stopped & (off_n == S)).any()  # ... beside stop-rejected samples that touch nobody
    assert best["index"] >= 0 and not stopped[best["index"]]
    nb = _np_best(on, np.repeat(lin, len(ang)), None, np.tile(ang, len(lin)))
    assert nb["index"] == best["index"]
    # score_one / score_one_crowd on a rejected sample that touches nobody, on one in contact and on an accepted sample: the
    # grid's entry; the Trajectory and the predicted crowd end where they end with the check off
    picks = (int(np.flatnonzero(stopped & (off_n == S))[0]), int(np.flatnonzero(both)[0]), int(best["index"]))
    want = {}
    g.set_stop_check(None)
    for t in picks:
        vx, vth = float(lin[t // len(ang)]), float(ang[t % len(ang)])
        want[t] = (len(g.score_one(scene.robot_state, vx, 0.0, vth, scene.goal_args)[1]),
                   g.score_one_crowd(scene.robot_state, vx, 0.0, vth, scene.goal_args))
    g.set_stop_check(check)
    for t in picks:
        vx, vth = float(lin[t // len(ang)]), float(ang[t % len(ang)])
        c1, p1 = g.score_one(scene.robot_state, vx, 0.0, vth, scene.goal_args)
        assert _same(c1, on[t]) and len(p1) == want[t][0] == off_n[t], (t, c1, on[t], len(p1), want[t][0], off_n[t])
        cw = g.score_one_crowd(scene.robot_state, vx, 0.0, vth, scene.goal_args)
        assert _same(cw["cost"], on[t]) and cw["n_steps"] == want[t][1]["n_steps"], (t, cw["cost"], on[t], cw["n_steps"])
        assert _same(cw["state"], want[t][1]["state"]) and _same(cw["work"], want[t][1]["work"])
    t = picks[1]
    assert want[t][1]["n_steps"] == off_n[t] < S
    g.close()


def test_with_people_prefix_levels(hip_mod, monkeypatch):
    """a grid large enough for the shared-prefix levels: the tail runs on the side stream beside them"""
    from sfw_test_util import _params as _scene_params
    scene = _people_scene(20)
    g = hip_mod.HipScorer(_scene_params())
    g.load_scene(scene)
    lin, ang = np.linspace(0.0, 0.7, 96), np.linspace(-0.5, 0.5, 96)
    off, _ = g.score_grid(scene.robot_state, lin, ang, scene.goal_args)
    info = g.plan_info()
    assert info["levels"] > 0, info
    g.set_stop_check((0.25, 0.25, 1.0, 256))
    on, best = g.score_grid(scene.robot_state, lin, ang, scene.goal_args)
    assert g.plan_info()["levels"] > 0
    steps, hit = g.stop_info(0, len(on))
    stopped = (hit >= 0) | (hit == SFW_STOP_UNFINISHED)
    assert stopped.any() and (~stopped & (off >= 0)).any()
    assert np.all(on[stopped] == -1.0) and _same(on[~stopped], off[~stopped])
    assert not stopped[best["index"]]
    g.close()


# ---- 5. containers -----------------------------------------------------------------------------------------------------------------------
def test_batch_member_with_the_check_takes_its_own_path(hip_mod, monkeypatch):
    monkeypatch.setenv("SFW_CYCLE_FUSED", "1")
    cases = [c for c in SR.wall_cases() if c.name in ("S2_tail3", "S6_tail20", "S6_reverse")]
    bs = hip_mod.BatchScorer(_params(2, SR.WALL_DT), 0, 3)
    singles = []
    for i, case in enumerate(cases):
        h = bs.member(i)
        _load(h, case, case.S)
        if i == 1:
            h.set_stop_check((*case.dec, case.max_steps))
        bs.stage(i, case.rs, case.lin, case.ang, case.goal)
        s = hip_mod.HipScorer(_params(case.S, case.dt))
        _load(s, case, case.S)
        if i == 1:
            s.set_stop_check((*case.dec, case.max_steps))
        singles.append((s.score_grid(case.rs, case.lin, case.ang, case.goal), s.stop_info(0, len(case.lin)) if i == 1 else None))
        s.close()
    bs.launch()
    bests = bs.fetch()
    d = bs.describe()
    assert d["one_launch_members"] == 2 and d["own_path_members"] == 1, d
    for i, case in enumerate(cases):
        (costs, best), rec = singles[i]
        assert _same(bs._costs(i), costs) and bests[i] == best, case.name
        if rec is not None:
            got = bs.member(i).stop_info(0, len(costs))
            assert np.array_equal(got[0], rec[0]) and np.array_equal(got[1], rec[1]) and (costs == -1.0).any()
    bs.close()


def test_ensemble_rejects_the_single_handles_set(hip_mod):
    from sfw_test_util import _params as _scene_params
    scene = _people_scene(5)
    lin, ang = np.linspace(0.0, 0.7, 7), np.linspace(-0.5, 0.5, 9)
    check = (0.25, 0.25, 1.0, 256)
    g = hip_mod.HipScorer(_scene_params())
    g.load_scene(scene)
    g.set_stop_check(check)
    single, _ = g.score_grid(scene.robot_state, lin, ang, scene.goal_args)
    _, hit = g.stop_info(0, len(single))
    g.close()
    stopped = (hit >= 0) | (hit == SFW_STOP_UNFINISHED)
    assert stopped.any()
    e = hip_mod.EnsembleScorer(_scene_params(), 0, 2)
    e.load_scene(scene, [scene.agents, scene.agents])
    e.set_stop_check(SfwStopCheck(*check, 0))
    for m in range(2):
        assert e.member(m).stop_check() == check
    for mode in ("mean", "max"):
        out = e.score_grid(scene.robot_state, lin, ang, scene.goal_args, mode=mode)
        costs = np.asarray(out[0])
        assert np.array_equal(costs == -1.0, single == -1.0), mode
    e.set_risk(tail_mass=0.5, contact_mass=0.25)
    out = e.score_grid(scene.robot_state, lin, ang, scene.goal_args, mode="mean")
    assert np.all(np.asarray(out[0])[stopped] == -1.0)
    assert np.array_equal(np.asarray(out[0]) == -1.0, single == -1.0)
    e.close()


def test_mppi_run_equals_the_loop_of_single_calls(hip_mod):
    """two iterations of the chain against its definition, call by call (as tests/test_mppi_gpu.py _loop), with the check on"""
    from sfw_test_util import _nominal, _params as _scene_params
    scene = _people_scene(5)
    K, n, seed, lam, gamma = 3, 96, 5, 0.5, 0.1
    nominal, sigma, lo, hi = _nominal(K), (0.15, 0.05, 0.3), (0.0, -0.3, -0.5), (0.7, 0.3, 0.5)
    ks, ga = (0, 7, 19), (1.0, 1.0, 1.0, scene.goal_args[3], scene.goal_args[4])
    check = (0.25, 0.25, 1.0, 256)

    def scorer():
        g = hip_mod.HipScorer(_scene_params())
        g.load_scene(scene)
        g.set_stop_check(check)
        return g
    a, b = scorer(), scorer()
    stats, plans, best = a.mppi_run(scene.robot_state, n, seed, nominal, sigma, lo, hi, ks, ga, 2, lam, gamma)
    nom, w_stats, w_plans, w_best = np.array(nominal, dtype=np.float64), [], [], None
    for i in range(2):
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
    assert _same(ca, cb)
    for g in (a, b):
        _, hit = g.stop_info(0, n)
        assert np.array_equal(ca == -1.0, hit != SFW_STOP_NONE)
    assert ((hit >= 0) | (hit == SFW_STOP_UNFINISHED)).any() and (hit == SFW_STOP_NONE).any(), hit
    a.close()
    b.close()


# ---- 6. state and errors -----------------------------------------------------------------------------------------------------------------
def test_state_and_errors(hip_mod, monkeypatch):
    monkeypatch.setenv("SFW_CYCLE_FUSED", "1")
    case = next(c for c in SR.wall_cases() if c.name == "S6_tail20")
    ref = SR.wall_reference(case)
    g = hip_mod.HipScorer(_params(case.S, case.dt))
    _load(g, case, case.S)
    assert g.stop_check() is None
    good = (0.1, 0.1, 0.1, 64)
    g.set_stop_check(good)
    L = hip_mod.lib()
    for bad in ((math.nan, 0.1, 0.1, 64, 0), (0.1, math.inf, 0.1, 64, 0), (0.1, 0.1, -1e-300, 64, 0), (0.1, 0.1, 0.1, 0, 0),
                (0.1, 0.1, 0.1, SFW_STOP_MAX_STEPS + 1, 0), (0.1, 0.1, 0.1, -1, 0), (0.1, 0.1, 0.1, 64, 1)):
        with pytest.raises(hip_mod.SfwError) as e:
            g.set_stop_check(SfwStopCheck(*bad))
        assert e.value.status == SFW_ERR_INVALID_ARG
        assert g.stop_check() == good
    import ctypes as C
    c = SfwStopCheck(*good, 0)
    assert L.sfw_set_stop_check(None, C.byref(c)) != 0 and L.sfw_get_stop_check(None, C.byref(c), None) != 0
    g.set_stop_check((0.0, 0.0, 0.0, SFW_STOP_MAX_STEPS))  # a limit of 0 and the largest max_steps are accepted
    assert g.stop_check() == (0.0, 0.0, 0.0, SFW_STOP_MAX_STEPS)
    g.set_stop_check(None)
    with pytest.raises(hip_mod.SfwError):
        g.stop_info(0, 1)  # before a stage
    with pytest.raises(hip_mod.SfwError):
        g.stop_points(0, 1, 4)
    # a stage with the check off: refused; a setter call between stage and launch does not affect that launch
    g.stage(case.rs, case.lin, case.ang, case.goal)
    g.set_stop_check((*case.dec, case.max_steps))
    g.launch()
    off = g.fetch()[0]
    assert np.all(np.asarray(off) >= 0.0)
    assert g.plan_info()["one_launch"] == 1
    with pytest.raises(hip_mod.SfwError):
        g.stop_info(0, len(case.lin))
    # ... and the other way round: staged with the check, switched off before the launch
    g.stage(case.rs, case.lin, case.ang, case.goal)
    g.set_stop_check(None)
    with pytest.raises(hip_mod.SfwError):
        g.stop_info(0, len(case.lin))  # staged, not launched yet
    g.launch()
    on = g.fetch()[0]
    want_rej = np.array([w[0] for w in ref.want])
    assert np.array_equal(np.asarray(on) == -1.0, want_rej) and want_rej.any()  # (A == 0: the cost scan_finish wrote is overwritten)
    steps, hit = g.stop_info(0, len(case.lin))
    assert np.array_equal(steps, ref.steps)
    # steps_cap smaller than the tail: only steps_cap poses, the full length all the same
    pts, n_steps = g.stop_points(0, len(case.lin), 3)
    assert pts.shape == (len(case.lin), 3, 3) and np.array_equal(n_steps, ref.steps) and n_steps.max() > 3
    for j in range(3):
        live = j < ref.steps
        assert RR.same_but_zero_sign(pts[live, j], ref.poses[j][live])
    for args in ((-1, 1, 4), (0, 0, 4), (0, len(case.lin) + 1, 4), (0, 1, 0)):
        with pytest.raises(hip_mod.SfwError):
            g.stop_points(*args)
    with pytest.raises(hip_mod.SfwError):
        g.stop_info(0, len(case.lin) + 1)
    # UNFINISHED under a limit of 0
    g.set_stop_check((0.0, 0.0, 0.0, 5))
    zero, _ = g.score_grid(case.rs, case.lin, case.ang, case.goal)
    steps, hit = g.stop_info(0, len(case.lin))
    assert np.all(np.asarray(zero) == -1.0) and np.all(hit == SFW_STOP_UNFINISHED) and np.all(steps == 5)
    g.close()


# ---- 7. the C++ host mirror ----------------------------------------------------------------------------------------------------------------
def _walled_scene(x_lo, x_hi):
    """the reference's 5 x 9 scene without people and with a lethal wall across the map at x_lo .. x_hi metres ahead"""
    import dataclasses

    from social_force_window_planner_amd import synthetic as syn
    scene = syn.make_scene(dataclasses.replace(syn.WORKLOADS["ref5x9"], n_people=0))
    c0, c1 = (int(round((x - scene.origin_x) / scene.resolution)) for x in (x_lo, x_hi))
    scene.cells[:] = 0
    scene.cells[:, c0:c1] = 254
    return scene


def test_host_mirror_hands_the_check_down(hip_mod):
    from social_force_window_planner_amd import host, synthetic as syn
    from social_force_window_planner_amd._abi import BRANCH_APPROACH, BRANCH_GRID, BRANCH_GRID_FAILED, default_ctrl_params
    host.build()
    lin, ang = syn.reference_sampler()
    vx, vth = np.repeat(lin, len(ang)), np.tile(ang, len(lin))
    pose, vel = [0.0, 0.0, 0.0], [0.3, 0.0, 0.0]
    ctrl = dict(max_trans_acc=0.5, max_rot_acc=1.0)
    # the grid branch: a wall 1.2 m ahead, beyond every rollout, inside the braking path of the faster samples
    scene = _walled_scene(1.2, 1.3)
    far_plan = [[x, 0.0, 0.0] for x in np.linspace(0.0, 4.0, 17)]
    plain, switched = host.HostPlanner(default_ctrl_params(**ctrl), scene), host.HostPlanner(default_ctrl_params(**ctrl), scene)
    for pl in (plain, switched):
        pl.update_plan(far_plan)
    off = plain.find_best_action(pose, vel)
    off_costs = plain.last_costs()
    assert off[2] == BRANCH_GRID and off[0]
    switched.set_stop_check(True, 512)
    on = switched.find_best_action(pose, vel)
    on_costs = switched.last_costs()
    stopped = (on_costs == -1.0) & (off_costs >= 0.0)
    assert on[2] == BRANCH_GRID and on[0] and stopped.any() and (on_costs >= 0.0).any()
    assert _same(on_costs[~stopped], off_costs[~stopped])
    nb = _np_best(on_costs, vx, None, vth)
    assert not stopped[nb["index"]] and on[1].tolist() == [vx[nb["index"]], 0.0, vth[nb["index"]]]
    # ... and the same verdicts as a handle given the controller's limits itself
    g = hip_mod.HipScorer(default_params(sim_time=1.0, sim_granularity=0.025))
    g.load_scene(scene)
    g.set_stop_check((0.5, 0.5, 1.0, 512))
    rs = tuple(float(np.float32(v)) for v in (*pose, *vel))
    costs, _ = g.score_grid(rs, lin, ang, (0.5, 0.0, 1.0, float(far_plan[switched.wp_index][0]), float(far_plan[switched.wp_index][1])))
    assert np.array_equal(np.asarray(costs) == -1.0, on_costs == -1.0)
    g.close()
    # switched off again: the check-off cycle, bit for bit
    switched.set_stop_check(False)
    again = switched.find_best_action(pose, vel)
    assert again[0] == off[0] and again[2] == off[2] and _same(again[1], off[1]) and _same(switched.last_costs(), off_costs)
    for pl in (plain, switched):
        pl.close()
    # the approach branch: the goal 1 m ahead (inside dist_thres), the wall right behind it; the approach command's own rollout
    # is legal, its braking path is not: with the check the scalar call (:299) refuses it and the cycle falls through to the grid
    scene = _walled_scene(0.95, 1.05)
    near_plan = [[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [1.0, 0.0, 0.0]]
    plain, checked = host.HostPlanner(default_ctrl_params(**ctrl), scene), host.HostPlanner(default_ctrl_params(**ctrl), scene)
    checked.set_stop_check(True, 512)
    for pl in (plain, checked):
        pl.update_plan(near_plan)
    off, on = plain.find_best_action(pose, vel), checked.find_best_action(pose, vel)
    assert off[2] == BRANCH_APPROACH and off[0]
    assert on[2] in (BRANCH_GRID, BRANCH_GRID_FAILED), on
    for pl in (plain, checked):
        pl.close()
