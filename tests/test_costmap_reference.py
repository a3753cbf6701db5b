"""tests/costmap_reference.py held to what it restates, on any machine: the recorded walks of the reference's LineIterator, the
oracle's footprint cost on every launch the GPU test runs (tests/test_costmap_edges_gpu.py), and the case lists held to their
purpose — they must contain coordinates at which the kernels' reciprocal product truncates differently from the division."""
import os

import numpy as np
import pytest

import costmap_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
AXIS_GEOMETRIES = [n for n in R.GEOMETRIES]


def _all_specs():
    out = []
    for n in AXIS_GEOMETRIES:
        out += R.address_specs(n)
    for n in R.POLY_GEOMETRIES:
        out += R.polygon_specs(n)
    return out + R.random_specs() + R.segment_specs() + R.illegal_specs()


def _poses(sp):
    return R.rollout(sp.rs, *R.samples(sp), sp.S)


def test_line_cells_equal_the_recorded_reference_walks():
    z = np.load(os.path.join(HERE, "golden", "reference", "line_iterator.npz"))
    at = 0
    for (x0, y0, x1, y1), n, first in zip(z["ends"].tolist(), z["lengths"].tolist(), z["first"].tolist()):
        codes = z["steps"][at:at + n - 1].astype(int)
        at += n - 1
        want = [tuple(first)]
        for c in codes:
            want.append((want[-1][0] + c // 3 - 1, want[-1][1] + c % 3 - 1))
        assert R.line_cells(x0, y0, x1, y1) == want, (x0, y0, x1, y1)
    assert at == len(z["steps"]) and len(z["ends"]) > 50


def test_line_cells_shape():
    for dx, dy in R.SEGMENTS:
        cells = R.line_cells(3, 4, 3 + dx, 4 + dy)
        assert cells[0] == (3, 4) and cells[-1] == (3 + dx, 4 + dy) and len(cells) == max(abs(dx), abs(dy)) + 1
    octants = {(np.sign(dx), np.sign(dy), abs(dx) > abs(dy)) for dx, dy in R.SEGMENTS if dx and dy and abs(dx) != abs(dy)}
    assert len(octants) == 8
    assert any(abs(dx) == abs(dy) and dx for dx, dy in R.SEGMENTS) and (0, 0) in R.SEGMENTS


@pytest.fixture(scope="module")
def oracle(oracle_mod):
    from social_force_window_planner_amd._abi import default_params

    return oracle_mod.OracleScorer(default_params())


def _against_oracle(oracle, specs):
    n = 0
    for sp in specs:
        oracle.set_costmap(sp.map.cells, sp.map.origin_x, sp.map.origin_y, sp.map.resolution)
        oracle.set_footprint(sp.footprint)
        seen = set()
        for x, y, th in _poses(sp).reshape(-1, 3).tolist():
            if (x, y, th) in seen or not (np.isfinite(x) and np.isfinite(y)):
                continue
            seen.add((x, y, th))
            if R.in_doubt(sp.map, sp.footprint, x, y, th):
                continue
            assert R.pose_code(sp.map, sp.footprint, x, y, th) == oracle.footprint_cost(x, y, th), (sp.name, x, y, th)
            n += 1
    return n


@pytest.mark.parametrize("gname", AXIS_GEOMETRIES)
def test_point_footprint_codes_equal_the_oracle(oracle, gname):
    assert _against_oracle(oracle, R.address_specs(gname)) > 100 or "x1" in gname or "1x" in gname


@pytest.mark.parametrize("gname", R.POLY_GEOMETRIES)
def test_polygon_codes_equal_the_oracle(oracle, gname):
    assert _against_oracle(oracle, R.polygon_specs(gname)) > 1000


def test_random_segment_and_illegal_codes_equal_the_oracle(oracle):
    assert _against_oracle(oracle, R.random_specs() + R.segment_specs() + R.illegal_specs()) > 4000


def test_every_code_class_occurs():
    """the launches reach every class of footprint code, and samples that are rejected behind legal steps"""
    seen, n_points = set(), set()
    for sp in R.illegal_specs() + R.polygon_specs(R.POLY_GEOMETRIES[0]):
        for v in R.expected(sp, _poses(sp)):
            if v is not None:
                n_points.add((sp.S, v[1]))
        for x, y, th in _poses(sp).reshape(-1, 3).tolist():
            seen.add((len(sp.footprint) >= 3, R.pose_code(sp.map, sp.footprint, x, y, th)))
    assert {(False, 252), (False, R.LETHAL), (False, R.UNKNOWN), (True, 253), (True, R.LETHAL), (True, R.UNKNOWN), (True, R.OFF_MAP)} <= seen
    assert {(5, 1), (5, 2), (5, 3), (5, 4), (5, 5)} <= n_points


def test_segment_launches_mark_what_they_say():
    """pose 1 of a segment launch's sample sees the marked cell exactly when its cell is on the footprint's walks"""
    n_hit = n_miss = 0
    for sp in R.segment_specs():
        for (x, y, th), hit in zip(_poses(sp)[:, 1].tolist(), sp.hits):
            assert R.pose_code(sp.map, sp.footprint, x, y, th) == (200 if hit else 0), sp.name
            n_hit, n_miss = n_hit + hit, n_miss + (not hit)
        assert R.pose_code(sp.map, sp.footprint, *sp.rs[:3]) == 0
    assert n_hit > 100 and n_miss > 300


def _axis_offsets():
    """{resolution: offsets a = w - origin >= 0 whose cell matters (up to one cell beyond the border)} over every coordinate the
    launches convert: centres, and vertices at heading 0"""
    out = {}
    for sp in _all_specs():
        m = sp.map
        poses = _poses(sp).reshape(-1, 3)
        level = poses[poses[:, 2] == 0.0]
        for p, (qx, qy) in [(poses, (0.0, 0.0))] + ([(level, q) for q in sp.footprint.tolist()] if len(sp.footprint) >= 3 else []):
            for w, q, o, size in ((p[:, 0], qx, m.origin_x, m.size_x), (p[:, 1], qy, m.origin_y, m.size_y)):
                with np.errstate(over="ignore", invalid="ignore"):
                    a = (w + q) - o  # (qx * 1 - qy * 0 == qx, qx * 0 + qy * 1 == qy)
                    a = a[(a >= 0) & (a / m.resolution < size + 1)]
                out.setdefault(m.resolution, []).append(a)
    return {r: np.unique(np.concatenate(v)) for r, v in out.items()}


def test_the_case_lists_tell_the_guarded_product_from_the_unguarded():
    offsets = _axis_offsets()
    assert {0.05, 0.1, 0.025, 0.03, R.THIRD, 0.07, 0.5, 4.0} <= set(offsets)
    for res, a in offsets.items():
        want = R.cell_index_division(a, res)
        assert np.array_equal(R.cell_index_guarded(a, res), want), res
        differ = int(np.sum(R.cell_index_product(a, res) != want))
        print(f"resolution {res!r}: {len(a)} offsets, the unguarded product truncates {differ} of them differently")
        if res in (0.5, 4.0):
            assert differ == 0  # (the reciprocal of a power of two is exact)
        else:
            assert differ > 0, res


def test_random_heading_cases_leave_out_at_most_one_percent():
    for sp in R.random_specs():
        tally = {}
        got = R.expected(sp, _poses(sp), tally)
        assert tally["poses"] >= 1500 and tally["left_out"] <= 0.01 * tally["poses"], tally
        legal = sum(1 for v in got if v is not None and not v[0])
        assert 100 <= legal <= len(got) - 100, legal  # both verdicts are well represented
        print(f"{sp.name}: {tally['left_out']} of {tally['poses']} poses left out, {legal} of {len(got)} samples legal")
