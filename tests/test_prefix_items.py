"""Work items of the shared-prefix levels (sfw_plan_shared_prefix_items: no handle, no device).  A level ending at step p
reads the robot's records of steps 0..p-1; a record holds the position after its step, which takes the heading BEFORE the step
(ref sfw_planner.cpp:586-588), so the records depend on the linear velocities of steps 0..p-1 and on the angular velocities of
steps 0..p-2 only: items = row classes(p) x column classes(p - 1), one column class for p = 1.  Checked against a Python
restatement of the recurrence, and against the robot's rollout itself (tests/rollout_reference.py): the lag is one step, not
none and not two."""
import ctypes as C

import numpy as np
import pytest

import rollout_reference as rr
from sfw_test_util import _bits, _new_velocity
from social_force_window_planner_amd import planner
from social_force_window_planner_amd import synthetic as syn


def _plans(lin, ang, vx0, vth0, acc_x, acc_th, sim_time, S, A, cap=64):
    """(ends, velocity classes) of sfw_plan_shared_prefix and (ends, items) of sfw_plan_shared_prefix_items"""
    L = planner.lib()
    lin, ang = np.ascontiguousarray(lin, dtype=np.float64), np.ascontiguousarray(ang, dtype=np.float64)
    out = []
    for fn in (L.sfw_plan_shared_prefix, L.sfw_plan_shared_prefix_items):
        fn.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                       C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        fn.restype = C.c_int
        ends, counts, n = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int64), C.c_int32(-1)
        assert fn(lin.ctypes.data, len(lin), ang.ctypes.data, len(ang), vx0, vth0, acc_x, acc_th, sim_time, S, A,
                  ends.ctypes.data, counts.ctypes.data, cap, C.byref(n)) == 0
        out.append(([int(v) for v in ends[:n.value]], [int(v) for v in counts[:n.value]]))
    return out


def _n_classes(targets, v0, a_max, dt, p):
    """Distinct sequences of the first p velocities (bit patterns); p = 0: nothing compared, one class."""
    seqs = set()
    for vg in targets:
        v, seq = v0, []
        for _ in range(p):
            v = _new_velocity(float(vg), v, a_max, dt)
            seq.append(np.float64(v).tobytes())
        seqs.add(tuple(seq))
    return len(seqs)


def _check(lin, ang, vx0, vth0, acc_x, acc_th, sim_time, S, A):
    (ends, classes), (ends_i, items) = _plans(lin, ang, vx0, vth0, acc_x, acc_th, sim_time, S, A)
    assert ends_i == ends  # one plan, counted twice
    dt = sim_time / S
    for p, n_cls, n_it in zip(ends, classes, items):
        rows = _n_classes(lin, vx0, acc_x, dt, p)
        assert n_it == rows * _n_classes(ang, vth0, acc_th, dt, p - 1)
        assert n_cls == rows * _n_classes(ang, vth0, acc_th, dt, p)
        assert n_it <= n_cls
    return ends, items


@pytest.mark.parametrize("name", ["cfg2", "target"])
def test_items_of_the_baseline_workloads(name):
    w = syn.WORKLOADS[name]
    scene = syn.make_scene(w)
    ends, items = _check(scene.linvels, scene.angvels, scene.robot_state[3], scene.robot_state[5], scene.goal_args[0],
                         scene.goal_args[2], w.sim_time, w.n_steps, w.n_people + 1)
    assert len(ends) >= 1 and items == sorted(items) and items[-1] < w.nv * w.nw


def test_items_of_degenerate_windows():
    """The windows of test_prefix_plan.py::test_degenerate_windows"""
    lin, ang = syn.generalised_sampler(64, 64)
    assert _check(lin, ang, 0.3, 0.0, 0.0, 0.0, 1.0, 40, 21) == ([39], [1])          # no acceleration: one class for ever
    assert _check(lin, ang, 0.3, 0.0, 1e6, 1e6, 1.0, 40, 21) == ([], [])             # everything reached in the first step
    lin2 = np.concatenate([lin, lin])
    # duplicate linear targets never separate; the angular targets are all distinct from the first step on, which the items
    # see one step late — never at a level's end, since every level ends at p >= 2 here
    assert _check(lin2, ang, 0.3, 0.0, 1e6, 1e6, 1.0, 40, 21) == ([39], [64 * 64])
    ends, _ = _check(lin, ang, 0.3, 0.0, 0.05, 0.05, 10.0, 400, 21)                  # long horizons
    assert ends and ends[-1] <= 48


def test_items_of_random_windows():
    rng = np.random.default_rng(2026)
    shared = 0
    for _ in range(20):
        nv, nw = int(rng.integers(64, 97)), int(rng.integers(64, 97))
        lo, hi = sorted(rng.uniform(-0.2, 0.9, 2))
        lin = np.linspace(lo, hi + 0.05, nv)
        ang = np.linspace(-rng.uniform(0.2, 1.2), rng.uniform(0.2, 1.2), nw)
        if rng.random() < 0.3:
            ang = np.round(ang * 16) / 16 + 0.0  # duplicates among the columns
        S = int(rng.integers(8, 61))
        ends, _ = _check(lin, ang, float(rng.uniform(0.0, 0.7)), float(rng.uniform(-0.5, 0.5)), float(rng.choice([0.5, 1.0, 2.5])),
                         float(rng.choice([0.5, 1.0, 3.0])), S * 0.025, S, int(rng.integers(2, 80)))
        shared += bool(ends)
    assert shared >= 10  # the windows are ones that share


# ---- the robot's rollout itself: 12 x 12 samples ------------------------------------------------------------------------------
S12, DT12 = 16, 0.025
RS12 = (0.2, -0.1, 0.3, 0.3, 0.0, 0.1)  # x, y, theta, vx, vy, vtheta
ACC12 = (1.0, 0.0, 1.0)
LIN12 = np.linspace(0.0, 0.7, 12)
ANG12 = np.linspace(-0.5, 0.5, 12)


def _axis_levels(targets, v0, a_max, max_p):
    """Class ids [level][target] of the library's own axis classes (level p at index p - 1; past the last level every target is
    its own class, as the planner reads them)"""
    L = planner.lib()
    t = np.ascontiguousarray(targets, dtype=np.float64)
    counts, cls = np.zeros(max_p, dtype=np.int32), np.full((max_p, len(t)), -1, dtype=np.int32)
    nl = C.c_int32(-1)
    L.sfw_plan_axis_classes.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    assert L.sfw_plan_axis_classes(t.ctypes.data, len(t), v0, a_max, DT12, max_p, 0, counts.ctypes.data, cls.ctypes.data,
                                   C.byref(nl), None) == 0
    return lambda p: np.zeros(len(t), dtype=np.int32) if p < 1 else cls[min(p, nl.value) - 1]


@pytest.fixture(scope="module")
def grid12():
    """Records of the 144 samples: rec[i] = (x, y after step i, vx, vy of step i), the K1 -> K2 table's content, with numpy's
    cos / sin of the exact layer's headings (a function of the heading's bits alone, as the device's is)"""
    lin, ang = np.repeat(LIN12, 12), np.tile(ANG12, 12)
    cmds = np.stack([lin, np.zeros(144), ang], axis=1)
    r = rr.rollout(S12, DT12, RS12, ACC12, cmds)
    x, y = np.full(144, RS12[0]), np.full(144, RS12[1])
    rec = np.empty((S12, 4, 144))
    for i in range(S12):
        x = x + (r.vx[i] * np.cos(r.th[i])) * DT12
        y = y + (r.vx[i] * np.sin(r.th[i])) * DT12
        rec[i] = x, y, r.vx[i], r.vy[i]
    rec.setflags(write=False)
    return rec


def _members(row_cls, col_cls):
    """sample indices by (row class, column class)"""
    groups = {}
    for iv in range(12):
        for iw in range(12):
            groups.setdefault((int(row_cls[iv]), int(col_cls[iw])), []).append(iv * 12 + iw)
    return list(groups.values())


def test_members_of_an_item_share_the_records_of_its_steps_and_no_more(grid12):
    rows, cols = _axis_levels(LIN12, RS12[3], ACC12[0], S12 - 1), _axis_levels(ANG12, RS12[5], ACC12[2], S12 - 1)
    split_at_p = split_one_late = 0
    for p in range(1, S12):
        for m in _members(rows(p), cols(p - 1)):
            b = _bits(grid12[:p][:, :, m])
            assert np.all(b == b[:, :, :1]), p  # every record of steps < p, bit for bit
            split_at_p += len(m) > 1 and bool(np.any(_bits(grid12[p][:, m]) != _bits(grid12[p][:, m[:1]])))
        if p >= 2:  # a lag of two steps would merge samples whose records of step p - 1 differ
            for m in _members(rows(p), cols(p - 2)):
                split_one_late += len(m) > 1 and bool(np.any(_bits(grid12[p - 1][:, m]) != _bits(grid12[p - 1][:, m[:1]])))
    assert split_at_p > 0 and split_one_late > 0


def test_the_velocity_classes_of_a_level_are_finer_than_its_items(grid12):
    """cols(p) x rows(p), what sfw_plan_shared_prefix reports, splits samples whose records of steps < p are all equal"""
    rows, cols = _axis_levels(LIN12, RS12[3], ACC12[0], S12 - 1), _axis_levels(ANG12, RS12[5], ACC12[2], S12 - 1)
    assert any(len(_members(rows(p), cols(p))) > len(_members(rows(p), cols(p - 1))) for p in range(1, S12))
