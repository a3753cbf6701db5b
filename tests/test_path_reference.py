"""social_force_window_planner_amd/path.py — the numpy restatement of the path term the device is compared with bit for bit —
against the exact layer of tests/path_reference.py, within the forward-error bound derived there.  No GPU."""
from fractions import Fraction as F

import numpy as np
import pytest

import path_reference as PR
from sfw_test_util import _same
from social_force_window_planner_amd import path as P

CASES = PR.adversarial_cases() + PR.random_cases(3, 60)


def test_segment_records_are_the_header_s():
    xy = np.array([(0.1, 0.2), (0.8, 0.3), (0.8, 0.3), (-1.5, 2.25)])
    rec = P.segment_records(xy)
    assert rec.shape == (3, 5)
    for k in range(3):
        ax, ay, bx, by = xy[k, 0], xy[k, 1], xy[k + 1, 0], xy[k + 1, 1]
        ex, ey = bx - ax, by - ay
        len2 = ex * ex + ey * ey
        assert _same(rec[k], [ax, ay, ex, ey, 1.0 / len2 if len2 > 0 else 0.0])
    assert rec[1, 4] == 0.0 and rec[1, 2] == 0.0 and rec[1, 3] == 0.0  # the repeated point: a zero-length segment
    one = P.segment_records([(1.0, 2.0)])
    assert _same(one, [[1.0, 2.0, 0.0, 0.0, 0.0]])  # a one-point path: one zero-length segment
    # a record's inv is within 3 roundings of 1 / |e|^2: c = E^2 inv of the bound is 1 up to g(3)-ish
    for k in (0, 2):
        E2 = F(float(rec[k, 2])) ** 2 + F(float(rec[k, 3])) ** 2
        assert abs(E2 * F(float(rec[k, 4])) - 1) <= PR.g(4)


@pytest.mark.parametrize("name,pose,pts", CASES, ids=[c[0] for c in CASES])
def test_distance_within_the_derived_bound(name, pose, pts):
    rec = P.segment_records(pts)
    got = P.pose_distance(np.array([pose[0]]), np.array([pose[1]]), pts)[0]
    want, bound = PR.exact_D(pose[0], pose[1], rec)
    err = abs(F(float(got)) - want)
    print(f"{name}: D = {float(want):.17g}, error {float(err):.3e} of a bound of {float(bound):.3e}")
    assert err <= bound, (name, float(err), float(bound))
    assert got >= 0.0 and not np.signbit(got)
    # per segment as well, and the clamp's three branches give what the exact layer gives where the case is exact
    for r in rec:
        d = P.segment_distance(np.array([pose[0]]), np.array([pose[1]]), r)[0]
        w, b = PR.exact_d(pose[0], pose[1], r)
        assert abs(F(float(d)) - w) <= b, name


def test_exactly_representable_cases_are_exact():
    """where every intermediate is a double, the result is the exact one: on the segment 0, beyond an end the end's distance"""
    assert P.pose_distance(0.5, 0.5, [(0.0, 0.0), (1.0, 1.0)]) == 0.0
    assert P.pose_distance(-2.0, 0.25, [(0.0, 0.0), (1.0, 0.0)]) == 4.0 + 0.0625
    assert P.pose_distance(3.0, -0.25, [(0.0, 0.0), (1.0, 0.0)]) == 4.0 + 0.0625
    assert P.pose_distance(0.5, 2.0, [(0.0, 0.0), (1.0, 0.0)]) == 4.0
    assert P.pose_distance(4.0, 6.0, [(1.0, 2.0)]) == 25.0 == P.pose_distance(4.0, 6.0, [(1.0, 2.0), (1.0, 2.0)])


def test_running_minimum_is_order_independent():
    rng = np.random.default_rng(9)
    pts = rng.uniform(-3.0, 3.0, (17, 2))
    pts[8] = pts[7]
    rec = P.segment_records(pts)
    px, py = rng.uniform(-4.0, 4.0, 500), rng.uniform(-4.0, 4.0, 500)
    base = P.records_distance(px, py, rec)
    assert _same(base, P.pose_distance(px, py, pts))
    for _ in range(8):
        assert _same(P.records_distance(px, py, rec[rng.permutation(len(rec))]), base)
    assert _same(P.records_distance(px, py, rec[::-1]), base)


@pytest.mark.parametrize("S", [1, 3, 8, 40])
def test_term_within_the_derived_bound(S):
    rng = np.random.default_rng(S)
    for scale in (1.0, 1e-3, 1e6):
        path = rng.uniform(-3.0, 3.0, (5, 2)) * scale
        points = np.zeros((6, S, 3))
        points[:, :, :2] = rng.uniform(-4.0, 4.0, (6, S, 2)) * scale
        points[:, 0, :2] = points[0, 0, :2]  # pose 0 is the robot's own: the same for every sample
        got = P.path_term(points, None, path)
        rec = P.segment_records(path)
        for t in range(6):
            want, bound = PR.exact_p(points[t, :, :2], rec)
            err = abs(F(float(got[t])) - want)
            assert err <= bound, (S, scale, t, float(err), float(bound))
    # in step order: the sum is the left-to-right one, not numpy's pairwise one
    D = P.pose_distance(points[:, :, 0], points[:, :, 1], path)
    acc = np.zeros(6)
    for i in range(S):
        acc = acc + D[:, i]
    assert _same(got, acc / S)


def test_term_sentinels_and_add():
    path = [(0.0, 0.0), (1.0, 0.0)]
    points = np.zeros((3, 4, 3))
    points[:, :, 1] = 0.5
    p = P.path_term(points, np.array([4, 2, 0]), path)
    assert p[0] == 0.25 and p[1] == -1.0 and p[2] == -1.0
    costs = np.array([1.5, -1.0, -2.0, 3.0, 0.0])
    pv = np.array([0.25, 0.25, -2.0, -1.0, 0.5])
    out = P.add(costs, pv, -2.0)
    assert _same(out, [1.5 + -2.0 * 0.25, -1.0, -2.0, 3.0, -1.0])  # contact keeps -1; a sentinel p leaves the cost; negative weight
    assert _same(P.add(costs, pv, 0.0), [1.5, -1.0, -2.0, 3.0, 0.0])


def test_check_arguments():
    P.check_arguments([(0.0, 0.0)], -1.0)
    P.check_arguments(np.zeros((P.SFW_PATH_MAX_POINTS, 2)), 0.0)
    for xy, w, r in ((np.zeros((0, 2)), 1.0, 0), (np.zeros((P.SFW_PATH_MAX_POINTS + 1, 2)), 1.0, 0), ([(np.nan, 0.0)], 1.0, 0),
                     ([(0.0, np.inf)], 1.0, 0), ([(1.0000001e7, 0.0)], 1.0, 0), ([(0.0, 0.0)], np.inf, 0), ([(0.0, 0.0)], np.nan, 0),
                     ([(0.0, 0.0)], 1.0, 1)):
        with pytest.raises(ValueError):
            P.check_arguments(xy, w, r)
