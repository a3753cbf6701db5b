"""tests/rollout_reference.py against the CPU oracle, on any machine: the exact layer bit for bit, the high-precision layer within
its own model with glibc's 1 ulp in place of the device library's figure — so that what tests/test_rollout_gpu.py holds the kernels
to is itself held to a second implementation by another hand — and the share of samples the angle term's verdict leaves out,
asserted on the reference alone for the very case lists the GPU test runs."""
import ctypes as C
import math

import numpy as np
import pytest

import rollout_reference as R
from sfw_test_util import _bits, _same
from social_force_window_planner_amd._abi import SFW_ERR_INVALID_ARG, SfwAgent, default_params

FAMILIES = R.families()
UNIT = {"vel": dict(vel_weight=1.0), "distance": dict(distance_weight=1.0), "angle": dict(angle_weight=1.0)}


def _params(sp, **weights):
    w = dict(vel_weight=0.0, distance_weight=0.0, angle_weight=0.0, costmap_weight=0.0, social_weight=0.0)
    w.update(weights)
    return default_params(sim_time=sp.sim_time, sim_granularity=sp.sim_granularity, max_vel_x=sp.max_vel_x, **w)


def _picked(sp):
    return range(sp.n) if sp.n <= 64 else range(0, sp.n, 17)


@pytest.mark.parametrize("family", [f for f in FAMILIES if f != "sequences"])  # (the oracle scores one command per sample)
def test_reference_against_the_oracle(oracle_mod, family):
    worst = {"pose": 0.0, "distance": 0.0}
    for sp in FAMILIES[family]:
        r = R.reference(sp, R.SINCOS_ULP_LIBM, R.ATAN2_ULP_LIBM)
        o = oracle_mod.OracleScorer(_params(sp))
        o.set_costmap(*R.free_map(sp))
        o.set_footprint(np.zeros((0, 2)))
        o.set_agents((SfwAgent * 0)())
        goal_args = sp.acc + sp.goal
        for t in _picked(sp):
            cmd = sp.cmds[0, t]
            got = {}
            for term, w in UNIT.items():
                o.set_params(_params(sp, **w))
                got[term], pts = o.score_one(sp.rs, cmd[0], cmd[1], cmd[2], goal_args, points_cap=sp.S)
            assert pts.shape == (sp.S, 3), sp.name
            # exact layer: S (the point count), every heading, the vel term
            assert R.same_but_zero_sign(pts[:, 2], r.ex.th[:sp.S, t]), (sp.name, t)
            assert _same(got["vel"], r.vel[t]), (sp.name, t, got["vel"], r.vel[t])
            # high-precision layer: the poses before every step and the distance within the model
            ex_ = np.abs((pts[:, 0] - r.hp.x[:sp.S, t]) - r.hp.x_lo[:sp.S, t])
            ey_ = np.abs((pts[:, 1] - r.hp.y[:sp.S, t]) - r.hp.y_lo[:sp.S, t])
            assert np.all(ex_ <= r.bx[:sp.S, t]) and np.all(ey_ <= r.by[:sp.S, t]), (sp.name, t)
            derr = R.distance_error(r.hp, got["distance"])[t]
            assert derr <= r.dist_bound[t], (sp.name, t, derr, r.dist_bound[t])
            for e, b in ((ex_, r.bx[:sp.S, t]), (ey_, r.by[:sp.S, t])):
                if np.any(b > 0):
                    worst["pose"] = max(worst["pose"], float(np.max(e[b > 0] / b[b > 0])))
            if r.dist_bound[t] > 0:
                worst["distance"] = max(worst["distance"], float(derr / r.dist_bound[t]))
            # the angle term wherever the verdict is decided
            if r.decided[t]:
                assert _same(got["angle"], r.ang[t]), (sp.name, t, got["angle"], r.ang[t])
            if sp.line:  # exact layer throughout
                line = R.straight_line_poses(sp.S, sp.dt, sp.rs, r.ex)
                assert _same(pts[:, :2], line[:sp.S, t]) and got["angle"] == 0.0, (sp.name, t)
                assert _same(got["distance"], R.distance_term(sp.goal[0], sp.goal[1], line[sp.S, t, 0], line[sp.S, t, 1])[0]), (sp.name, t)
        o.close()
    print(f"{family}: largest error / model (glibc, 1 ulp): {worst}")


def test_step_count_against_the_oracle(oracle_mod):
    """the exact layer's S is sfwo_num_steps: the list of tests/test_oracle_kat.py, quotients one ulp either side of k + 0.5,
    sim_time = 0, the largest admitted count and what lies beyond it"""
    L = oracle_mod.lib()
    cases = [(1.0, 0.025), (1.5, 0.25), (2.0, 0.025), (0.5, 0.025), (0.01, 0.025), (0.0, 0.025), (0.1, 0.03)]
    for k in (0, 1, 7, 8, 40, 512, 4095, R.MAX_STEPS - 1):
        h = k + 0.5
        cases += [(np.nextafter(h, 0.0), 1.0), (h, 1.0), (np.nextafter(h, np.inf), 1.0), (np.nextafter(h, 0.0) * 0.025, 0.025)]
    cases += [(float(R.MAX_STEPS), 1.0), (np.nextafter(R.MAX_STEPS + 0.5, 0.0), 1.0), (R.MAX_STEPS * 2.0 ** -6, 2.0 ** -6)]
    for st, g in cases:
        got = L.sfwo_num_steps(C.byref(default_params(sim_time=float(st), sim_granularity=float(g))))
        assert got == R.num_steps(st, g) and 1 <= got <= R.MAX_STEPS, (st, g, got)
    assert R.num_steps(R.MAX_STEPS, 1.0) == R.MAX_STEPS and R.num_steps(0.0, 0.025) == 1
    for st, g in [(R.MAX_STEPS + 0.5, 1.0), (R.MAX_STEPS + 1.0, 1.0), (1e300, 1.0), (math.inf, 1.0), (1.0, 1e-300), (1.0, math.inf),
                  (math.nan, 1.0), (1.0, math.nan), (1.0, 0.0), (-1.0, 1.0), (1.0, -1.0)]:
        assert L.sfwo_num_steps(C.byref(default_params(sim_time=st, sim_granularity=g))) == SFW_ERR_INVALID_ARG, (st, g)
        with pytest.raises(ValueError):
            R.num_steps(st, g)


def test_float_normalize_angle_against_the_oracle(oracle_mod):
    L = oracle_mod.lib()
    vals = np.concatenate([R.standing_headings(), -R.standing_headings(), np.random.default_rng(5).uniform(-40, 40, 500)]).astype(np.float32)
    want = R.normalize_angle_f32(vals)
    got = np.array([L.sfwo_normalize_angle(float(v), float(R.F32_NEG_PI), float(R.F32_PI)) for v in vals], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_share_left_out_by_the_angle_verdict():
    """under the DEVICE library's figures and the GPU test's margin: the constructed families leave out no sample, the random
    family at most 1 % (expected: about 1e-7)"""
    for family, specs in FAMILIES.items():
        n = left = 0
        for sp in specs:
            r = R.reference(sp, R.SINCOS_ULP_DEVICE, R.ATAN2_ULP_DEVICE, 2.0)
            n += sp.n
            left += int(np.sum(~r.decided))
        print(f"{family}: {left} of {n} samples left out")
        assert left <= (0.01 * n if family == "general" else 0), (family, left, n)


def test_case_lists_are_what_they_claim():
    for family, specs in FAMILIES.items():
        assert len({sp.name for sp in specs}) == len(specs)
        for sp in specs:
            assert R.num_steps(sp.sim_time, sp.sim_granularity) == sp.S and R.step_dt(sp.sim_time, sp.S) == sp.dt, sp.name
            assert math.frexp(sp.dt)[0] in (0.0, 0.5), sp.name  # a power of two: a launch of S + 1 steps has S's poses as a prefix
            if sp.lin is not None:
                assert sp.K == 1 and np.array_equal(_bits(sp.cmds[0]), _bits(R.product(sp.lin, sp.ang))), sp.name
    assert sorted(sp.S for sp in FAMILIES["steps"] if sp.dt > 0 and sp.lin is not None) == sorted(R.STEP_COUNTS)
    # the ramp does what its targets are named after (acc = 1, start 0.25, vx of the samples whose other target is 0.25's)
    sp = next(s for s in FAMILIES["ramp"] if s.name == "ramp_x")
    vx = R.reference(sp, R.SINCOS_ULP_DEVICE, R.ATAN2_ULP_DEVICE, 2.0).ex.vx
    q = R.Q
    assert vx[14, 0] < 0.5 and vx[15, 0] == 0.5 and vx[19, 0] == 0.5           # above: reached by step 15's update
    assert vx[14, 1] > 0.0 and vx[15, 1] == 0.0                                 # below
    assert vx[1, 2] == 0.25 + 2 * q and vx[2, 2] == 0.25 + 3 * q == vx[3, 2]     # reached exactly on a step
    assert vx[1, 3] == 0.25 + 2 * q and vx[2, 3] == 0.25 + 2.5 * q == vx[19, 3]  # overshot, then clipped
    assert vx[19, 4] == 0.25 + 20 * q < 0.7                                     # never reached
    assert np.all(vx[:, 5] == 0.25)                                             # equal from step 0
    assert vx[19, 6] == 0.25 - 20 * q < 0.0 and np.all(vx[19, 7] == 0.0)        # through zero to the other sign; -0.0 (sign not compared)
    over = next(s for s in FAMILIES["ramp"] if s.name == "ramp_acc_overflow")
    assert np.isinf(np.float64(over.acc[0]) * over.dt) and np.array_equal(R.reference(over, 4.0, 6.0, 2.0).ex.vx[0], over.cmds[0, :, 0])
    tiny = next(s for s in FAMILIES["ramp"] if s.name == "ramp_acc_dbl_min")
    assert tiny.acc[0] * tiny.dt == np.finfo(np.float64).tiny
    # a sequence's knot takes over AT its step
    sp = next(s for s in FAMILIES["sequences"] if s.knot_steps == (0, 7, 8, 9))
    ex = R.rollout(sp.S, sp.dt, sp.rs, (1e300,) * 3, sp.cmds, sp.knot_steps)  # unlimited: the velocity IS the active target
    for step, k in ((6, 0), (7, 1), (8, 2), (9, 3), (19, 3)):
        assert np.array_equal(ex.vx[step], sp.cmds[k, :, 0]), step
