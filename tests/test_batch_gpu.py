"""Many planners' control cycles in one launch (sfw_batch_*, csrc/sfw_kernels.hip sfw_batch_cycle_kernel): every member's
costs, sentinels, selection, captured Trajectory points and point counts are bit for bit those of a standalone handle on the
same scene, whatever mix of crowds, scans, groups, grids, step counts and precisions the batch holds."""
import dataclasses

import numpy as np
import pytest

from social_force_window_planner_amd import synthetic as syn
from social_force_window_planner_amd._abi import (SFW_ERR_STATE, SFW_OK, SFW_PRECISION_F32, SFW_PRECISION_F64,
                                                   SFW_PRECISION_F64_STRICT, default_params)
from sfw_test_util import _same

pytestmark = pytest.mark.gpu

# (people, laser points, nv, nw, steps, groups)
MIX = [(5, 0, 5, 9, 40, False), (0, 16, 3, 7, 6, False), (20, 60, 5, 9, 40, True), (1, 0, 32, 32, 6, False),
       (50, 240, 5, 9, 1, False), (62, 0, 3, 7, 40, False), (8, 16, 5, 9, 6, True)]


@dataclasses.dataclass
class Member:
    scene: object
    params: object
    robot_state: tuple
    goal_args: tuple


def _member(i, people=5, obs=0, nv=5, nw=9, steps=40, groups=False, precision=SFW_PRECISION_F64, seed=0):
    gran = 0.025 if steps >= 40 else 0.25 if steps <= 6 else 0.05
    w = dataclasses.replace(syn.WORKLOADS["ref5x9"], n_people=people, n_obstacles=obs, sim_time=steps * gran,
                            sim_granularity=gran, seed=100 + 7 * i + seed)
    if (nv, nw) != (5, 9):
        w = dataclasses.replace(w, nv=nv, nw=nw, sampler="generalised")
    scene = syn.make_scene(w)
    if groups:
        for a in range(1, min(people, 7) + 1):
            scene.agents[a].group_id = 1 + (a % 2)
    x, y, th, vx, vy, vth = scene.robot_state
    rs = (x + 0.01 * i, y - 0.005 * i, th + 0.02 * i, vx * (1.0 - 0.03 * (i % 5)), vy, vth + 0.01 * (i % 3))
    acc_x, acc_y, acc_th, wpx, wpy = scene.goal_args
    ga = (acc_x, acc_y, acc_th, wpx + 0.1 * (i % 4), wpy - 0.05 * (i % 3))
    p = default_params(sim_time=w.sim_time, sim_granularity=w.sim_granularity, precision=precision)
    return Member(scene, p, rs, ga)


def _mix(B, **kw):
    return [_member(i, *MIX[i % len(MIX)], **kw) for i in range(B)]


def _alone(hip_mod, m, capture=True):
    g = hip_mod.HipScorer(m.params)
    g.load_scene(m.scene)
    g.set_points_capture(capture)
    costs, best = g.score_grid(m.robot_state, m.scene.linvels, m.scene.angvels, m.goal_args)
    pts, n = g.grid_points_batch(0, len(costs), m.scene.workload.n_steps)
    g.close()
    return costs, best, pts, n


def _load(bs, members, capture=True):
    for i, m in enumerate(members):
        h = bs.member(i)
        h.set_params(m.params)
        h.load_scene(m.scene)
        h.set_points_capture(capture)


def _batched(bs, members):
    for i, m in enumerate(members):
        bs.stage(i, m.robot_state, m.scene.linvels, m.scene.angvels, m.goal_args)
    bs.launch()
    bests = bs.fetch()
    out = []
    for i, m in enumerate(members):
        h = bs.member(i)
        costs = h.costs_view().copy()
        pts, n = h.grid_points_batch(0, len(costs), m.scene.workload.n_steps)
        out.append((costs, bests[i], pts, n))
    return out


def _check(got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        assert _same(a[0], b[0]), (i, np.flatnonzero(a[0] != b[0]))
        assert a[1] == b[1], (i, a[1], b[1])
        assert np.array_equal(a[3], b[3]) and _same(a[2], b[2]), i


@pytest.mark.parametrize("B", [1, 2, 7, 32])
def test_mixed_members_equal_their_own_launches(hip_mod, B):
    members = _mix(B)
    want = [_alone(hip_mod, m) for m in members]
    bs = hip_mod.BatchScorer(default_params(), 0, B)
    _load(bs, members)
    _check(_batched(bs, members), want)
    d = bs.describe()
    one = [bs.member(i).plan_info() for i in range(B)]  # (the staged grids: what a launch of each alone would be)
    assert d["members"] == B and d["one_launch_members"] == sum(p["one_launch"] for p in one) >= 1
    assert d["own_path_members"] == B - d["one_launch_members"] and d["batch_launches"] >= 1
    assert d["batch_blocks"] == sum(p["samples"] for p in one if p["one_launch"])
    bs.close()


def test_three_precisions_one_launch_each(hip_mod):
    members = [_member(i, people=6, obs=0, precision=p) for i, p in
               enumerate([SFW_PRECISION_F64, SFW_PRECISION_F32, SFW_PRECISION_F64_STRICT] * 3)]
    want = [_alone(hip_mod, m) for m in members]
    bs = hip_mod.BatchScorer(default_params(), 0, len(members))
    _load(bs, members)
    _check(_batched(bs, members), want)
    d = bs.describe()
    assert d["batch_launches"] == 3 and d["one_launch_members"] == len(members)


def test_homogeneous_fleet_is_one_launch(hip_mod):
    B = 22
    members = [_member(i) for i in range(B)]
    want = [_alone(hip_mod, m) for m in members]
    bs = hip_mod.BatchScorer(members[0].params, 0, B)
    _load(bs, members)
    _check(_batched(bs, members), want)
    d = bs.describe()
    assert d["batch_launches"] == 1 and d["one_launch_members"] == B and d["own_path_members"] == 0
    assert d["batch_blocks"] == 45 * B
    # the one-call form: common grid, per-member robot states and goals
    res = bs.score_grid([m.robot_state for m in members], members[0].scene.linvels, members[0].scene.angvels,
                        [m.goal_args for m in members])
    for (c, b), w in zip(res, want):
        assert _same(c, w[0]) and b == w[1]
    assert bs.last_us()["stage"] > 0.0


def test_mixed_qualification(hip_mod):
    members = _mix(5)
    members.append(_member(5, people=5, nv=64, nw=64, steps=6))   # 4096 samples: not a control cycle's grid
    members.append(_member(6, people=99, obs=0, steps=6))         # A = 100: register form, not the cycle kernel
    want = [_alone(hip_mod, m, capture=False) for m in members]
    bs = hip_mod.BatchScorer(default_params(), 0, len(members))
    _load(bs, members, capture=False)
    got = _batched(bs, members)
    _check(got, want)
    d = bs.describe()
    assert d["own_path_members"] == 2 and d["one_launch_members"] == 5


def test_consecutive_launches_interleaved_with_single_scores(hip_mod):
    members = _mix(7)
    want = [_alone(hip_mod, m) for m in members]
    bs = hip_mod.BatchScorer(default_params(), 0, len(members))
    _load(bs, members)
    for rnd in range(3):
        _check(_batched(bs, members), want)
        m = members[rnd]
        costs, best = bs.member(rnd).score_grid(m.robot_state, m.scene.linvels, m.scene.angvels, m.goal_args)
        assert _same(costs, want[rnd][0]) and best == want[rnd][1]


def test_changed_costmap_on_some_members(hip_mod):
    members = _mix(6)
    bs = hip_mod.BatchScorer(default_params(), 0, len(members))
    _load(bs, members)
    _batched(bs, members)
    for i in (1, 4):  # a new map on these members: the copy path; the others hand over the same map (direct arena fetch)
        cells = members[i].scene.cells.copy()
        cells[: cells.shape[0] // 3, :] = 254
        members[i] = dataclasses.replace(members[i], scene=dataclasses.replace(members[i].scene, cells=cells))
    for i, m in enumerate(members):
        bs.member(i).set_costmap(m.scene.cells, m.scene.origin_x, m.scene.origin_y, m.scene.resolution)
    want = [_alone(hip_mod, m) for m in members]
    _check(_batched(bs, members), want)


def test_cycle_fused_off(hip_mod, monkeypatch):
    members = _mix(7)
    want = [_alone(hip_mod, m) for m in members]
    monkeypatch.setenv("SFW_CYCLE_FUSED", "0")
    bs = hip_mod.BatchScorer(default_params(), 0, len(members))
    _load(bs, members)
    _check(_batched(bs, members), want)
    assert bs.describe()["one_launch_members"] == 0 and bs.describe()["batch_launches"] == 0


def test_state_errors_then_a_good_batch(hip_mod):
    L = hip_mod.lib()
    members = _mix(3)
    want = [_alone(hip_mod, m) for m in members]
    bs = hip_mod.BatchScorer(default_params(), 0, 3)
    _load(bs, members)
    assert L.sfw_batch_launch(bs._b) == SFW_ERR_STATE  # nothing staged
    assert b"member 0" in L.sfw_batch_last_error(bs._b)
    for i, m in enumerate(members[:2]):
        bs.stage(i, m.robot_state, m.scene.linvels, m.scene.angvels, m.goal_args)
    assert L.sfw_batch_launch(bs._b) == SFW_ERR_STATE
    assert b"member 2" in L.sfw_batch_last_error(bs._b)
    m = members[2]
    bs.stage(2, m.robot_state, m.scene.linvels, m.scene.angvels, m.goal_args)
    bs.member(2).score_one(m.robot_state, 0.3, 0.0, 0.1, m.goal_args)  # consumes the staged grid
    assert L.sfw_batch_launch(bs._b) == SFW_ERR_STATE
    assert b"member 2" in L.sfw_batch_last_error(bs._b)
    assert L.sfw_destroy(L.sfw_batch_member(bs._b, 0)) == SFW_ERR_STATE
    # a failing stage inside the one-call form launches nothing
    bad = [m.robot_state for m in members]
    bad[1] = (float("nan"),) + tuple(bad[1][1:])
    with pytest.raises(hip_mod.SfwError):
        bs.score_grid(bad, members[0].scene.linvels, members[0].scene.angvels, [m.goal_args for m in members])
    _check(_batched(bs, members), want)
    assert L.sfw_batch_fetch(bs._b, None) == SFW_OK


def test_members_against_the_oracle(hip_mod):
    from oracle.sfw_oracle import OracleScorer

    members = [_member(i, *MIX[j]) for i, j in enumerate((0, 1, 3, 5))]
    bs = hip_mod.BatchScorer(default_params(), 0, len(members))
    _load(bs, members)
    got = _batched(bs, members)
    for m, (costs, best, _, _) in zip(members, got):
        o = OracleScorer(m.params)
        o.load_scene(m.scene)
        oc, ob = o.score_grid(m.robot_state, m.scene.linvels, m.scene.angvels, m.goal_args)
        assert np.array_equal(oc < 0, costs < 0)
        v = oc >= 0
        if v.any():
            assert np.max(np.abs(costs[v] - oc[v]) / np.abs(oc[v])) <= 1e-9
        assert best["index"] == ob["index"]


def test_create_destroy_returns_memory(hip_mod):
    import torch

    free0, _ = torch.cuda.mem_get_info(0)
    m = _member(0)
    for _ in range(20):
        bs = hip_mod.BatchScorer(m.params, 0, 64)
        _load(bs, [m] * 64)
        _batched(bs, [m] * 64)
        bs.close()
    free1, _ = torch.cuda.mem_get_info(0)
    assert free0 - free1 <= 64 << 20, (free0, free1)
