"""The stop check's references against each other, on the CPU: the package's numpy restatement (stop.py) equals
tests/stop_reference.py bit for bit, the constructed tails have the lengths worked out by hand, and the "wall ahead" family
that tests/test_stop_check_gpu.py runs through every kernel path holds every kind of sample by the references alone."""
import math

import numpy as np
import pytest

import rollout_reference as RR
import stop_reference as SR
from social_force_window_planner_amd import stop as P

DT = 2.0 ** -6


def _tails(end, dec, dt, max_steps):
    return SR.exact_tail(end, dec, dt, max_steps), P.tail(end, dec, dt, max_steps)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_package_restatement_equals_the_reference(seed):
    rng = np.random.default_rng(seed)
    n = 200
    end = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-math.pi, math.pi, n), rng.uniform(-0.7, 0.7, n),
                    rng.uniform(-0.3, 0.3, n), rng.uniform(-0.5, 0.5, n)], axis=1)
    end[::7, 4] = 0.0   # no lateral velocity
    end[::11, 3] = 0.0  # vy alone
    end[::77, 3:5] = 0.0  # at rest: no tail
    dec = (rng.uniform(0.5, 2.0), rng.uniform(0.2, 1.0), rng.uniform(0.5, 2.0))
    for max_steps in (5, 4096):
        a, b = _tails(end, dec, DT, max_steps)
        assert np.array_equal(a.steps, b.steps) and np.array_equal(a.unfinished, b.unfinished)
        m = a.vx.shape[0]
        live = np.arange(m)[:, None] < a.steps[None, :]
        for name in ("vx", "vy", "vth"):
            assert RR.same_but_zero_sign(np.where(live, getattr(a, name), 0.0), np.where(live, getattr(b, name), 0.0)), name
        assert RR.same_but_zero_sign(np.where(live, a.th[1:], 0.0), np.where(live, b.th, 0.0))  # the heading pose j is checked at
        assert (a.steps == 0).sum() >= 2 and a.steps.max() > 5 or max_steps == 5
    assert a.unfinished.sum() == 0


def test_straight_poses_are_exact_in_both():
    end = np.array([[0.2, -0.1, 0.0, v, 0.0, 0.0] for v in (0.7, 0.3, -0.25, 0.0, 1e-3)])
    a, b = _tails(end, (0.4, 0.4, 0.4), 0.25, 64)
    pa = SR.straight_tail_poses(end, a, 0.25)
    live = np.arange(pa.shape[0])[:, None] < a.steps[None, :]
    for c, got in enumerate((b.x, b.y, b.th)):
        assert RR.same_but_zero_sign(np.where(live, pa[:, :, c], 0.0), np.where(live, got, 0.0))


def _steps(v, dec, dt, max_steps, axis=3):
    end = np.zeros((1, 6))
    end[0, axis] = v
    a, b = _tails(end, dec, dt, max_steps)
    assert a.steps[0] == b.steps[0] and a.unfinished[0] == b.unfinished[0]
    return int(a.steps[0]), bool(a.unfinished[0])


def test_constructed_tail_lengths():
    one = (1.0, 1.0, 1.0)
    q = 1.0 * DT  # the velocity step: a power of two, so k * q is exact
    # a limit of 0 on a moving axis: never brakes, UNFINISHED at max_steps; on an axis at rest it does not matter
    assert _steps(0.3, (0.0, 1.0, 1.0), DT, 17) == (17, True)
    assert _steps(0.3, (1.0, 0.0, 0.0), DT, 4096)[1] is False
    # an exact multiple of dec * dt and its two neighbouring doubles: k steps, k steps (one rounding below), k + 1 steps
    k = 13
    v = k * q
    assert _steps(v, one, DT, 4096) == (k, False)
    assert _steps(float(np.nextafter(v, 0.0)), one, DT, 4096) == (k, False)
    assert _steps(float(np.nextafter(v, 1.0)), one, DT, 4096) == (k + 1, False)
    # a negative velocity brakes upwards: the same lengths (the reference's `> 0.0` loop would not have run at all)
    assert _steps(-v, one, DT, 4096) == (k, False)
    assert _steps(float(np.nextafter(-v, -1.0)), one, DT, 4096) == (k + 1, False)
    # vy alone
    assert _steps(v, one, DT, 4096, axis=4) == (k, False)
    assert _steps(v, (1.0, 0.5, 1.0), DT, 4096, axis=4) == (2 * k, False)
    # vtheta alone does not make a tail: the robot turns on the spot
    assert _steps(0.5, one, DT, 4096, axis=5) == (0, False)
    # max_steps reached exactly at standstill is a finished tail; one step earlier it is not
    assert _steps(v, one, DT, k) == (k, False)
    assert _steps(v, one, DT, k - 1) == (k - 1, True)
    assert _steps(v, one, DT, 1) == (1, True)
    assert _steps(q, one, DT, 1) == (1, False)


def test_argument_checks_of_the_restatement():
    for dec, ms, res in (((math.nan, 1, 1), 4, 0), ((1, math.inf, 1), 4, 0), ((1, 1, -1e-300), 4, 0), ((1, 1, 1), 0, 0),
                         ((1, 1, 1), SR.MAX_STEPS + 1, 0), ((1, 1, 1), 4, 1)):
        with pytest.raises(ValueError):
            P.check_arguments(dec, ms, res)
    P.check_arguments((0.0, 0.0, 0.0), SR.MAX_STEPS)
    P.check_arguments((1.0, 1.0, 1.0), 1)


def test_verdict_of_the_restatement_equals_the_reference():
    for case in SR.wall_cases():
        ref = SR.wall_reference(case)
        tl = ref.tail
        illegal = np.zeros(tl.vx.shape, dtype=bool)
        for j in range(illegal.shape[0]):
            for i in range(illegal.shape[1]):
                code = SR.CR.pose_code(case.map, case.footprint, ref.poses[j, i, 0], ref.poses[j, i, 1], ref.poses[j, i, 2])
                illegal[j, i] = code < 0 or code >= 254
        rejected, hit = P.verdict(tl.steps, tl.unfinished, illegal)
        want = SR.verdict(case.map, case.footprint, np.transpose(ref.poses, (1, 0, 2)), tl.steps, tl.unfinished)
        assert [(bool(r), int(h)) for r, h in zip(rejected, hit)] == want, case.name


def test_wall_family_holds_every_kind():
    """by the references alone: accepted, rejected by a lethal cell, rejected off the map, UNFINISHED; tails of 0, 1, 3 and
    about 20 steps; every sample legal with the check off"""
    kinds, lengths = set(), set()
    for case in SR.wall_cases():
        ref = SR.wall_reference(case)
        assert 5 <= len(case.lin) <= 12 and case.S in (2, 6)
        # with the check off every sample of the family has a cost >= 0, as a grid / list and as a two-knot sequence
        assert not ref.rejected_costmap.any() and not SR.wall_reference(case, sequence=True).rejected_costmap.any(), case.name
        for i, (rejected, hit) in enumerate(ref.want):
            if ref.skipped[i]:
                continue
            lengths.add(int(ref.steps[i]))
            if not rejected:
                kinds.add("accepted")
            elif hit == SR.UNFINISHED:
                kinds.add("unfinished")
            else:
                x, y, th = ref.poses[hit, i]
                code = SR.CR.pose_code(case.map, case.footprint, x, y, th)
                kinds.add("off_map" if code == -3 else "lethal")
                assert code in (-3, -1), (case.name, i, code)
        per_case = {("r" if w[0] else "a") for w, s in zip(ref.want, ref.skipped) if not s}
        print(case.name, sorted(per_case), sorted(set(int(s) for s in ref.steps)))
    assert kinds == {"accepted", "lethal", "off_map", "unfinished"}, kinds
    assert {0, 1, 3} <= lengths and any(18 <= n <= 24 for n in lengths), sorted(lengths)


@pytest.mark.parametrize("gname,fname,seed,holonomic", SR.RANDOM_CASES)
def test_random_cases_stay_within_the_doubt_cap(gname, fname, seed, holonomic):
    """the seeds of the GPU test's random-heading launches, by the references alone (the exact layer's end state at the
    high-precision pose, numpy's cos and sin): at most 1 % of the tail poses are in doubt, tails of several steps, no sample
    UNFINISHED, and both verdicts occur among the samples whose rollout is legal"""
    case = SR.random_case(gname, fname, seed, holonomic)
    ex, tl, hp, bx, by = SR.random_reference(case)
    S, n = case.S, len(case.cmds)
    assert not tl.unfinished.any() and tl.steps.min() >= 1 and tl.vx.shape[0] >= 4
    assert (np.any(case.cmds[:, 1] != 0.0)) == holonomic and case.rs[5] != 0.0
    assert float(bx.max()) < 1e-9 and float(by.max()) < 1e-9  # the bound is far below the 1e-6 m margin of in_doubt
    end = SR.end_state(ex, S, np.stack([hp.x[S], hp.y[S]], axis=1))
    t = P.tail(end, case.dec, case.dt, case.max_steps)
    assert np.array_equal(t.steps, tl.steps)
    legal = np.ones(n, dtype=bool)
    for i in range(n):
        for s in range(S):
            code = SR.CR.pose_code(case.map, case.footprint, hp.x[s, i], hp.y[s, i], ex.th[s, i])
            if code < 0 or code >= 254:
                legal[i] = False
                break
    poses = np.stack([t.x, t.y, t.th], axis=2).transpose(1, 0, 2)
    tally = {}
    want = SR.verdict(case.map, case.footprint, poses, np.where(legal, tl.steps, 0), np.zeros(n, dtype=bool), tally)
    kinds = {w[0] for w, ok in zip(want, legal) if ok and w is not None}
    print(case.name, tally, int(legal.sum()), kinds)
    assert tally["left_out"] <= 0.01 * tally["poses"] and tally["poses"] >= 300, tally
    assert legal.sum() >= n // 2 and kinds == {True, False}
