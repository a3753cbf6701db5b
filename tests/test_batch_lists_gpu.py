"""List, sequence and perturbed members of a batch in ONE launch (sfw_batch_set_list_fusion; csrc/sfw_kernels.hip
sfw_batch_cycle_list_kernel / sfw_batch_cycle_seq_kernel).

Every comparison is bitwise (uint64 views), against the same member scored alone on a standalone handle with the same world:
the cost vector, sfw_best and its key, n_valid, the captured terms [n, 5], the captured Trajectory points and point counts, and
the sfw_grid_crowd rows (whose length is the contact step) of one valid and one rejected sample where the member has them.
Scenes are 5 x 5 m maps (100 cells of 0.05 m) with 12 steps of 1/16 s, except where a case is about the step count or about a
chunked table."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from social_force_window_planner_amd import synthetic as syn
from social_force_window_planner_amd._abi import (SFW_ERR_INVALID_ARG, SFW_OK, SFW_PERTURB_KEEP_NORMALS, SFW_PRECISION_F32,
                                                   SFW_PRECISION_F64, SFW_PRECISION_F64_STRICT, SFW_SEQ_MAX_KNOTS, SfwAgent, SfwBest,
                                                   SfwGoalArgs, SfwPerturb, SfwRobotState, default_params)
from sfw_test_util import _bits, _nominal, _same

pytestmark = pytest.mark.gpu

GRAN = 0.0625
S = 12
HOLO_GA = (1.0, 0.7, 1.0, 2.0, 0.5)
STEPS3 = (0, 2, 50)  # the last knot lies beyond the horizon
SIGMA = (0.2, 0.1, 0.3)
WIDE = ((0.0, -0.3, -0.5), (0.7, 0.3, 0.5))
KEEP = SFW_PERTURB_KEEP_NORMALS
L4 = [0.01, 0.1, 1.0, 10.0]


def _params(precision=SFW_PRECISION_F64, steps=S):
    return default_params(sim_time=steps * GRAN, sim_granularity=GRAN, precision=precision)


@functools.lru_cache(maxsize=None)
def _scene(people, seed, obs=0, groups=False, kind=None):
    """(cached and never written to)"""
    base = syn.make_scene(syn.Workload("t", 1, 1, people, 100, S * GRAN, sim_granularity=GRAN, seed=seed, n_obstacles=obs, n_discs=0,
                                       footprint="point" if kind else "polygon16"))
    if groups:
        for a in range(1, min(people, 6) + 1):
            base.agents[a].group_id = a % 2
    if kind is None:
        return base
    # one slow person 0.5 m ahead on the robot's axis: a robot that advances 0.15 m touches it (contact radius 0.35 m)
    agents = (SfwAgent * len(base.agents))()
    for a in range(len(base.agents)):
        C.memmove(C.byref(agents[a]), C.byref(base.agents[a]), C.sizeof(SfwAgent))
    p = agents[1]
    p.x, p.y, p.vx, p.vy, p.has_goal, p.desired_velocity = 0.5, 0.0, 0.0, 0.0, 0, 0.05
    cells = base.cells.copy()
    my = int((0.0 - base.origin_y) / base.resolution)
    if kind == "illegal":  # the robot stands on a lethal cell: every pose from step 0 on is illegal
        p.x = 3.0
        cells[:, :] = 254
    elif kind == "contact_then_illegal":  # ... and a lethal block from x = 0.25 m: reached two or three steps after the contact
        mx = int((0.25 - base.origin_x) / base.resolution)
        cells[my - 2:my + 2, mx:mx + 3] = 254
    else:
        assert kind == "contact"
    return dataclasses.replace(base, cells=cells, agents=agents)


def _commands(n, seed, K=1, forward=False):
    rng = np.random.default_rng(seed)
    vx = rng.uniform(0.5, 0.7, (K, n)) if forward else rng.uniform(0.0, 0.7, (K, n))
    vth = np.zeros((K, n)) if forward else rng.uniform(-0.5, 0.5, (K, n))
    vy = np.zeros((K, n)) if forward else rng.uniform(-0.3, 0.3, (K, n))
    return vx, vy, vth


@dataclasses.dataclass
class Member:
    scene: object
    params: object
    rs: tuple
    ga: tuple
    kind: str        # "grid" | "list" | "seq" | "pert"
    n: int
    K: int = 1
    cmd: tuple = None      # (vx, vy, vth), (K, n) arrays
    steps: tuple = (0,)
    pert: dict = None      # seed, nominal, sigma, lo, hi, flags
    steps_n: int = S       # the launch's step count

    def stage(self, h):
        if self.kind == "grid":
            h.stage(self.rs, self.scene.linvels, self.scene.angvels, self.ga)
        elif self.kind == "list":
            h.stage_samples(self.rs, self.cmd[0][0], self.cmd[2][0], self.ga, vy=self.cmd[1][0])
        elif self.kind == "seq":
            h.stage_sequences(self.rs, self.cmd[0], self.cmd[2], self.steps, self.ga, vy=self.cmd[1])
        else:
            q = self.pert
            h.stage_perturbed(self.rs, self.n, q["seed"], q["nominal"], q["sigma"], q["lo"], q["hi"], self.steps, self.ga,
                              flags=q.get("flags", 0))


def _member(i, kind, n, people=5, obs=0, groups=False, precision=SFW_PRECISION_F64, K=3, steps=STEPS3, scene_kind=None,
            forward=False, flags=0, steps_n=S):
    scene = _scene(people, 300 + people, obs, groups, scene_kind)
    x, y, th, vx, vy, vth = scene.robot_state
    rs = (x + 0.01 * i, y - 0.005 * i, th + 0.02 * i, vx, vy, vth + 0.01 * (i % 3)) if scene_kind is None else scene.robot_state
    ga = (HOLO_GA[0], 0.0 if forward else HOLO_GA[1], HOLO_GA[2], HOLO_GA[3] + 0.1 * (i % 4), HOLO_GA[4] - 0.05 * (i % 3))
    m = Member(scene, _params(precision, steps_n), rs, ga, kind, n, steps_n=steps_n)
    if kind == "grid":
        lin, ang = syn.reference_sampler()
        m.scene = dataclasses.replace(scene, linvels=lin, angvels=ang)
        m.ga = scene.goal_args
    elif kind == "list":
        m.cmd = _commands(n, 900 + i, 1, forward)
    elif kind == "seq":
        m.K, m.steps, m.cmd = K, tuple(steps[:K]), _commands(n, 900 + i, K, forward)
    else:
        m.K, m.steps = K, tuple(steps[:K]) if K <= 3 else tuple(range(K))
        nominal = _nominal(K)
        nominal[:, 0] += 0.02 * i
        box = (tuple(v + 0.01 * (i % 3) for v in WIDE[0]), tuple(v - 0.01 * (i % 2) for v in WIDE[1]))
        m.pert = dict(seed=7000 + 13 * i, nominal=nominal, sigma=SIGMA, lo=box[0], hi=box[1], flags=flags)
    return m


def _load(h, m):
    h.set_params(m.params)
    h.load_scene(m.scene)
    h.set_points_capture(True)
    h.set_terms_capture(True)


def _snapshot(h, m, best=None):
    """Everything a launch leaves on handle h, after the wait"""
    costs, b, key = h.fetch()
    if best is not None:
        assert best == b, (best, b)
    T = len(costs)
    snap = {"costs": costs, "best": b, "key": np.array(key, dtype=np.float64), "terms": h.cost_terms()}
    snap["points"], snap["n_points"] = h.grid_points_batch(0, T, m.steps_n)
    valid, rejected = np.flatnonzero(costs >= 0), np.flatnonzero(costs == -1.0)
    for name, idx in (("valid", valid), ("rejected", rejected)):
        if len(idx):
            d = h.grid_crowd(int(idx[0]))
            for k, v in d.items():
                snap[f"crowd_{name}_{k}"] = v
    if m.kind == "pert":
        snap["knots"] = h.knots(0, m.n)
        if m.pert.get("flags", 0) & KEEP:
            snap["normals"] = h.normals(0, m.n)
    return snap


def _diff(a, b):
    """names of the entries of two snapshots that are not bit for bit the same"""
    bad = [k for k in set(a) ^ set(b)]
    for k in set(a) & set(b):
        x, y = a[k], b[k]
        if isinstance(x, dict):
            ok = x == y and all(_same(x[f], y[f]) for f in ("cost", "vx", "vy", "vtheta"))
        elif isinstance(x, np.ndarray) and x.dtype == np.float64:
            ok = _same(x, y)
        elif isinstance(x, np.ndarray):
            ok = np.array_equal(x, y)
        else:
            ok = _bits(float(x)).item() == _bits(float(y)).item()
        if not ok:
            bad.append(k)
    return sorted(bad)


_ALONE = {}


def _alone(hip_mod, m, tag=None):
    """the member's own launch on a standalone handle: computed once per tag, never written to"""
    if tag is not None and tag in _ALONE:
        return _ALONE[tag]
    g = hip_mod.HipScorer(m.params)
    _load(g, m)
    m.stage(g)
    g.launch()
    snap = _snapshot(g, m)
    g.close()
    if tag is not None:
        _ALONE[tag] = snap
    return snap


def _batch(hip_mod, members, fusion):
    bs = hip_mod.BatchScorer(_params(), 0, len(members))
    for i, m in enumerate(members):
        _load(bs.member(i), m)
    if fusion is not None:
        bs.set_list_fusion(fusion)
    return bs


def _launch(bs, members, restage=True):
    if restage:
        for i, m in enumerate(members):
            m.stage(bs.member(i))
    bs.launch()
    bests = bs.fetch()
    return [_snapshot(bs.member(i), m, bests[i]) for i, m in enumerate(members)]


def _hold(got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        assert _diff(a, b) == [], (i, _diff(a, b))


def _three_kinds():
    return [_member(0, "grid", 45), _member(1, "list", 7), _member(2, "seq", 7)]


# ---- 1. the default ----------------------------------------------------------------------------------------------------------------
def test_default_is_off(hip_mod):
    members = _three_kinds()
    bs = _batch(hip_mod, members, None)
    assert bs.list_fusion() == 0
    got = _launch(bs, members)
    d = bs.describe()
    assert d["members"] == 3 and d["one_launch_members"] == 1 and d["own_path_members"] == 2 and d["batch_launches"] == 1, d
    _hold(got, [_alone(hip_mod, m, ("kinds", i)) for i, m in enumerate(members)])
    bs.close()


# ---- 2. kinds ------------------------------------------------------------------------------------------------------------------------
def test_grid_list_and_sequences_are_one_launch_each(hip_mod):
    members = _three_kinds()
    bs = _batch(hip_mod, members, True)
    assert bs.list_fusion() == 1
    got = _launch(bs, members)
    plans = [bs.member(i).plan_info() for i in range(3)]
    assert all(p["one_launch"] for p in plans), plans
    d = bs.describe()
    assert d["one_launch_members"] == 3 and d["own_path_members"] == 0 and d["batch_launches"] == 3, d
    assert d["batch_blocks"] == sum(p["samples"] for p in plans) == 45 + 7 + 7 and d["lds_bytes"] > 0, d
    _hold(got, [_alone(hip_mod, m, ("kinds", i)) for i, m in enumerate(members)])
    assert any(len(np.flatnonzero(g["costs"] >= 0)) for g in got)
    bs.close()


# ---- 3. the member search and the member-local index -------------------------------------------------------------------------------
SIZES = [1, 3, 64, 65, 257, 1024, 2]
CROWDS = [61, 0, 1, 5, 20, 61, 5]  # A - 1 of member i


def _search_member(i):
    return _member(i, "seq", SIZES[i], people=CROWDS[i])


@pytest.mark.parametrize("order", ["forward", "reversed", "first", "first_two"])
def test_member_search_and_local_index(hip_mod, order):
    idx = {"forward": list(range(7)), "reversed": list(range(6, -1, -1)), "first": [5], "first_two": [5, 0]}[order]
    members = [_search_member(i) for i in idx]
    want = [_alone(hip_mod, m, ("search", i)) for i, m in zip(idx, members)]
    bs = _batch(hip_mod, members, True)
    got = _launch(bs, members)
    # (61 people on 64-double planes is the largest crowd of the list the one-kernel cycle accepts)
    assert all(bs.member(k).plan_info()["one_launch"] for k in range(len(idx)))
    d = bs.describe()
    assert d["batch_launches"] == 1 and d["one_launch_members"] == len(idx) and d["own_path_members"] == 0, d
    assert d["batch_blocks"] == sum(SIZES[i] for i in idx), d
    _hold(got, want)
    assert sum(len(np.flatnonzero(g["costs"] >= 0)) for g in got) > 0
    bs.close()


# ---- 4. variants -----------------------------------------------------------------------------------------------------------------------
def test_one_launch_per_precision_variant_and_kind(hip_mod):
    members = []
    for kind in ("list", "seq"):
        for j, (obs, groups, precision) in enumerate([(0, False, SFW_PRECISION_F64), (60, False, SFW_PRECISION_F64),
                                                      (0, True, SFW_PRECISION_F64), (0, False, SFW_PRECISION_F32),
                                                      (60, False, SFW_PRECISION_F64_STRICT), (0, False, SFW_PRECISION_F64),
                                                      (0, True, SFW_PRECISION_F32)]):
            members.append(_member(len(members), kind, 5 + j, people=6, obs=obs, groups=groups, precision=precision))
    want = [_alone(hip_mod, m) for m in members]
    bs = _batch(hip_mod, members, True)
    got = _launch(bs, members)
    d = bs.describe()
    # per kind: (f64, plain) twice, (f64, laser), (f64, groups), (f32, plain), (strict, laser), (f32, groups): six variants
    assert d["batch_launches"] == 12 and d["one_launch_members"] == len(members) and d["own_path_members"] == 0, d
    _hold(got, want)
    bs.close()


# ---- 5. perturbed members --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, KEEP])
def test_perturbed_members(hip_mod, flags):
    members = [_member(i, "pert", 65, K=4, flags=flags) for i in range(3)]
    alone = []
    for m in members:
        g = hip_mod.HipScorer(m.params)
        _load(g, m)
        m.stage(g)
        g.launch()
        snap = _snapshot(g, m)
        snap["blend"] = g.blend(L4, want_weights=True)
        snap["control"] = g.control_cost(0.3)
        alone.append(snap)
        g.close()
    bs = _batch(hip_mod, members, True)
    got = _launch(bs, members)
    d = bs.describe()
    assert d["batch_launches"] == 1 and d["one_launch_members"] == 3, d
    for i, m in enumerate(members):
        h = bs.member(i)
        b = got[i]["best"]
        assert b["index"] >= 0 and [b["vx"], b["vy"], b["vtheta"]] == list(got[i]["knots"][0, :, b["index"]]), (i, b)
        st, u, w = h.blend(L4, want_weights=True)
        ast, au, aw = alone[i].pop("blend")
        assert [sorted(x.items()) for x in st] == [sorted(x.items()) for x in ast] and _same(u, au) and _same(w, aw), i
        assert _same(h.control_cost(0.3), alone[i].pop("control")), i
    _hold(got, alone)
    bs.close()


# ---- 6. members that do not qualify ------------------------------------------------------------------------------------------------
def test_members_that_do_not_qualify_keep_their_own_path(hip_mod, monkeypatch):
    members = [_member(0, "seq", 9), _member(1, "list", 1025), _member(2, "seq", 3, steps_n=520), _member(3, "list", 9)]
    want = [_alone(hip_mod, m) for m in members]
    bs = _batch(hip_mod, members, True)
    got = _launch(bs, members)
    plans = [bs.member(i).plan_info()["one_launch"] for i in range(4)]
    assert plans == [1, 0, 0, 1], plans
    d = bs.describe()
    assert d["one_launch_members"] == 2 and d["own_path_members"] == 2 and d["batch_launches"] == 2, d
    _hold(got, want)
    # SFW_CYCLE_FUSED=0 (read at every launch): every member takes its own path
    monkeypatch.setenv("SFW_CYCLE_FUSED", "0")
    got = _launch(bs, members)
    d = bs.describe()
    assert d["one_launch_members"] == 0 and d["own_path_members"] == 4 and d["batch_launches"] == 0, d
    _hold(got, want)
    monkeypatch.delenv("SFW_CYCLE_FUSED")
    bs.close()
    # a member whose tables are chunked (the budget is read when the handle is created)
    chunked = [_member(0, "seq", 2100, steps_n=32), _member(1, "seq", 9)]
    want = [_alone(hip_mod, m) for m in chunked]
    monkeypatch.setenv("SFW_TABLE_BUDGET_MB", "1")
    bs = _batch(hip_mod, chunked, True)
    monkeypatch.delenv("SFW_TABLE_BUDGET_MB")
    got = _launch(bs, chunked)
    assert bs.member(0).plan_info()["chunks"] > 1
    d = bs.describe()
    assert d["one_launch_members"] == 1 and d["own_path_members"] == 1, d
    _hold(got, want)
    bs.close()


# ---- 7. rejections inside a member -----------------------------------------------------------------------------------------------------
def test_rejections_inside_a_member(hip_mod):
    members = [_member(0, "seq", 9),
               _member(1, "seq", 5, people=1, scene_kind="contact", forward=True),
               _member(2, "seq", 9),
               _member(3, "seq", 5, people=1, scene_kind="illegal", forward=True),
               _member(4, "seq", 5, people=1, scene_kind="contact_then_illegal", forward=True),
               _member(5, "seq", 9)]
    want = [_alone(hip_mod, m) for m in members]
    # the scenes are what they are meant to be (conditions on the scenes, read off the standalone launches)
    assert want[1]["best"]["index"] == -1 and want[1]["best"]["n_valid"] == 0 and np.all(want[1]["costs"] == -1.0)
    assert np.all(want[1]["n_points"] > 0) and np.all(want[1]["n_points"] < S)          # a contact inside the horizon
    assert np.all(want[3]["costs"] == -1.0) and np.all(want[3]["n_points"] == 0)          # illegal from step 0
    # (the CPU oracle on these scenes: the contact at step 5 for every vx in [0.5, 0.7], the block from x = 0.25 m behind it)
    assert np.all(want[4]["costs"] == -1.0) and np.all(want[4]["n_points"] > 0) and np.all(want[4]["n_points"] < S)
    assert all(want[i]["best"]["n_valid"] > 0 for i in (0, 2, 5))
    bs = _batch(hip_mod, members, True)
    got = _launch(bs, members)
    d = bs.describe()
    assert d["batch_launches"] == 1 and d["one_launch_members"] == 6, d
    _hold(got, want)
    _hold(_launch(bs, members, restage=False), want)  # the members' election counters came back to zero
    bs.close()


# ---- 8. re-launch ----------------------------------------------------------------------------------------------------------------------
def test_relaunch_and_the_switch_between_launches(hip_mod):
    members = [_member(0, "seq", 65), _member(1, "list", 9), _member(2, "pert", 33, K=4, flags=KEEP), _member(3, "grid", 45)]
    want = [_alone(hip_mod, m) for m in members]
    bs = _batch(hip_mod, members, True)
    _hold(_launch(bs, members), want)
    _hold(_launch(bs, members, restage=False), want)
    assert bs.describe()["one_launch_members"] == 4
    bs.set_list_fusion(False)
    _hold(_launch(bs, members, restage=False), want)
    d = bs.describe()
    assert d["one_launch_members"] == 1 and d["own_path_members"] == 3 and bs.list_fusion() == 0, d
    bs.set_list_fusion(True)
    _hold(_launch(bs, members, restage=False), want)
    assert bs.describe()["one_launch_members"] == 4 and bs.describe()["batch_launches"] == 3
    bs.close()


# ---- 9. the three score calls ----------------------------------------------------------------------------------------------------------
def _score_call_members(kind):
    if kind == "pert":
        return [_member(i, "pert", 33, K=3, flags=KEEP) for i in range(3)]
    return [_member(i, kind, 33) for i in range(3)]


@pytest.mark.parametrize("kind", ["list", "seq", "pert"])
@pytest.mark.parametrize("fusion", [False, True])
def test_score_calls_against_staging_by_hand(hip_mod, kind, fusion):
    members = _score_call_members(kind)
    want = [_alone(hip_mod, m, ("score", kind, i)) for i, m in enumerate(members)]
    bs = _batch(hip_mod, members, fusion)
    rs, ga = [m.rs for m in members], [m.ga for m in members]
    if kind == "pert":
        res = bs.score_perturbed(rs, 33, [m.pert for m in members], members[0].steps, ga)
    else:
        vx, vy, vth = (np.stack([m.cmd[c] for m in members]) for c in range(3))
        res = bs.score_samples(rs, vx[:, 0], vth[:, 0], ga, vy=vy[:, 0]) if kind == "list" else \
            bs.score_sequences(rs, vx, vth, members[0].steps, ga, vy=vy)
    assert bs.list_fusion() == int(fusion)  # (the calls honour the switch; they do not turn it on)
    d = bs.describe()
    assert d["one_launch_members"] == (3 if fusion else 0) and d["batch_launches"] == (1 if fusion else 0), d
    for i, (c, b) in enumerate(res):
        assert _same(c, want[i]["costs"]) and b == want[i]["best"], i
    _hold([_snapshot(bs.member(i), m) for i, m in enumerate(members)], want)
    assert bs.last_us()["stage"] > 0.0
    bs.close()


def test_score_calls_refuse_before_any_member_is_staged(hip_mod):
    L = hip_mod.lib()
    members = _score_call_members("seq")
    want = [_alone(hip_mod, m, ("score", "seq", i)) for i, m in enumerate(members)]
    bs = _batch(hip_mod, members, True)
    _launch(bs, members)
    B, n, K = 3, 33, 3
    rs = (SfwRobotState * B)(*[SfwRobotState(*m.rs) for m in members])
    ga = (SfwGoalArgs * B)(*[SfwGoalArgs(*m.ga) for m in members])
    best = (SfwBest * B)()
    vx, vy, vth = (np.ascontiguousarray(np.stack([m.cmd[c] for m in members])) for c in range(3))
    ks = np.array(members[0].steps, dtype=np.int32)
    seqs = {m: bs.member(m)._h.value for m in range(B)}

    def still_the_previous_launch(rc):
        assert rc == SFW_ERR_INVALID_ARG, rc
        assert L.sfw_batch_fetch(bs._b, best) == SFW_OK  # nothing was re-staged: the previous launch is still fetchable
        _hold([_snapshot(bs.member(i), m) for i, m in enumerate(members)], want)

    bad = vx.copy()
    bad[2, 1, 5] = np.nan  # a non-finite knot in member 2 of 3
    still_the_previous_launch(L.sfw_batch_score_sequences(bs._b, rs, bad.ctypes.data, vy.ctypes.data, vth.ctypes.data, n, K,
                                                          ks.ctypes.data, ga, best))
    assert b"member 2" in L.sfw_batch_last_error(bs._b)
    bad1, vth0 = np.ascontiguousarray(bad[:, 1]), np.ascontiguousarray(vth[:, 0])  # (B, n) lists; member 2 holds the NaN
    still_the_previous_launch(L.sfw_batch_score_samples(bs._b, rs, bad1.ctypes.data, None, vth0.ctypes.data, n, ga, best))
    assert b"member 2" in L.sfw_batch_last_error(bs._b)
    args = (vx.ctypes.data, vy.ctypes.data, vth.ctypes.data)
    not_ascending = np.array([0, 5, 5], dtype=np.int32)
    for call in (lambda: L.sfw_batch_score_sequences(bs._b, None, *args, n, K, ks.ctypes.data, ga, best),
                 lambda: L.sfw_batch_score_sequences(bs._b, rs, None, args[1], args[2], n, K, ks.ctypes.data, ga, best),
                 lambda: L.sfw_batch_score_sequences(bs._b, rs, *args, n, K, None, ga, best),
                 lambda: L.sfw_batch_score_sequences(bs._b, rs, *args, n, K, ks.ctypes.data, None, best),
                 lambda: L.sfw_batch_score_sequences(bs._b, rs, *args, 0, K, ks.ctypes.data, ga, best),
                 lambda: L.sfw_batch_score_sequences(bs._b, rs, *args, n, SFW_SEQ_MAX_KNOTS + 1, ks.ctypes.data, ga, best),
                 lambda: L.sfw_batch_score_sequences(bs._b, rs, *args, n, K, not_ascending.ctypes.data, ga, best),
                 lambda: L.sfw_batch_score_samples(bs._b, rs, args[0], None, None, n, ga, best),
                 lambda: L.sfw_batch_score_samples(bs._b, rs, args[0], None, args[2], 0, ga, best),
                 lambda: L.sfw_batch_score_samples(bs._b, None, args[0], None, args[2], n, ga, best),
                 lambda: L.sfw_batch_score_perturbed(bs._b, rs, None, n, K, ks.ctypes.data, ga, best),
                 lambda: L.sfw_batch_score_perturbed(bs._b, rs, (SfwPerturb * B)(), n, K, ks.ctypes.data, ga, best)):  # nominal NULL
        still_the_previous_launch(call())
    # perturbations: one member's sigma negative
    made = [hip_mod.HipScorer._perturb(7, _nominal(K), SIGMA, WIDE[0], WIDE[1], ks, 0) for _ in range(B)]
    pt = (SfwPerturb * B)(*[m[0] for m in made])
    pt[1].sigma[2] = -1.0
    still_the_previous_launch(L.sfw_batch_score_perturbed(bs._b, rs, pt, n, K, ks.ctypes.data, ga, best))
    assert b"member 1" in L.sfw_batch_last_error(bs._b)
    assert L.sfw_batch_score_sequences(None, rs, *args, n, K, ks.ctypes.data, ga, best) == SFW_ERR_INVALID_ARG
    # and a good call afterwards
    res = bs.score_sequences([m.rs for m in members], vx, vth, members[0].steps, [m.ga for m in members], vy=vy)
    for i, (c, b) in enumerate(res):
        assert _same(c, want[i]["costs"]) and b == want[i]["best"], i
    assert seqs == {m: bs.member(m)._h.value for m in range(B)}
    bs.close()
