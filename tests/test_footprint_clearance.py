"""The footprint clearance map's rule against the exact costmap reference, without a GPU.

The rule (tests/clearance_reference.py, what sfw_kernels.hip's two passes compute): a cell is clear when the whole window of
half-width r_c = ceil(R / res) + 1 around it is on the map and free.  What the kernels rely on (footprint_cost_clear): a pose
whose centre cell is clear has footprint code 0 by tests/costmap_reference.py, whatever its heading; and r_c is never smaller
than the largest per-axis offset between a vertex's cell and the centre's that the reference produces — measured here with
centres on cell edges (and their neighbouring doubles) and the farthest vertex pointing along an axis, the poses that reach
the bound's ceil(R / res) part."""
import math

import numpy as np
import pytest

import clearance_reference as CR
import costmap_reference as R

FOOTPRINTS = {"polygon16": R.polygon16(), "box": np.array(R.BOX), "k2": np.array(CR.K2_FOOTPRINT)}
RESOLUTIONS = [0.05, 0.03]
ORIGIN = (-0.85, 1.7)


def _maps(res, seed):
    """random maps of at most 64 x 48 cells, wide and tall: the first free, the others with one to four nonzero cells"""
    rng = np.random.default_rng(seed)
    out = []
    for k, (sx, sy) in enumerate(((64, 48), (48, 64), (57, 41))):
        cells = np.zeros((sy, sx), dtype=np.uint8)
        for _ in range(int(rng.integers(1, 5)) if k else 0):
            cells[rng.integers(0, sy), rng.integers(0, sx)] = rng.choice([1, 7, 200, 253, 254, 255])
        out.append(R.make_map(cells, ORIGIN[0], ORIGIN[1], res))
    return out


def _edge(rng, origin, res, size):
    """a coordinate on a cell edge of the axis, or one of its neighbouring doubles"""
    v = np.float64(origin) + np.float64(rng.integers(0, size + 1)) * np.float64(res)
    return float([np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)][int(rng.integers(0, 3))])


def _poses(m, fp, r, rng, n):
    """n poses (x, y, theta): uniform over the map and a margin, on cell edges, within r_c of each border, and with the
    farthest vertex turned onto each axis direction from a centre on a cell edge"""
    w, h = m.size_x * m.resolution, m.size_y * m.resolution
    out = []
    for _ in range(n // 4):
        out.append((m.origin_x + rng.uniform(-0.1, 1.1) * w, m.origin_y + rng.uniform(-0.1, 1.1) * h, rng.uniform(-math.pi, math.pi)))
    for _ in range(n // 4):
        out.append((_edge(rng, m.origin_x, m.resolution, m.size_x), _edge(rng, m.origin_y, m.resolution, m.size_y),
                    rng.choice([0.0, math.pi / 2, rng.uniform(-math.pi, math.pi)])))
    band = (r + 1.5) * m.resolution
    for _ in range(n // 4):
        x, y = m.origin_x + rng.uniform(0, 1) * w, m.origin_y + rng.uniform(0, 1) * h
        side = int(rng.integers(0, 4))
        if side == 0:
            x = m.origin_x + rng.uniform(0, band)
        elif side == 1:
            x = m.origin_x + w - rng.uniform(0, band)
        elif side == 2:
            y = m.origin_y + rng.uniform(0, band)
        else:
            y = m.origin_y + h - rng.uniform(0, band)
        out.append((x, y, rng.uniform(-math.pi, math.pi)))
    far = fp[int(np.argmax(np.hypot(fp[:, 0], fp[:, 1])))]
    turn = -math.atan2(far[1], far[0])  # the heading that puts the farthest vertex on +x
    for _ in range(n - 3 * (n // 4)):
        out.append((_edge(rng, m.origin_x, m.resolution, m.size_x), _edge(rng, m.origin_y, m.resolution, m.size_y),
                    turn + int(rng.integers(0, 4)) * math.pi / 2))
    return out


@pytest.mark.parametrize("res", RESOLUTIONS)
@pytest.mark.parametrize("fname", list(FOOTPRINTS))
def test_clear_poses_cost_zero_and_offsets_stay_in_the_window(fname, res):
    fp = FOOTPRINTS[fname]
    r = CR.half_width(fp, res)
    assert r is not None and r == math.ceil(float(np.max(np.hypot(fp[:, 0], fp[:, 1]))) / res) + 1
    rng = np.random.default_rng(1000 + k_seed(fname, res))
    n_clear = n_on_map = worst = 0
    for k, m in enumerate(_maps(res, 11 + k_seed(fname, res))):
        clear = CR.clearance_map(m.cells, r)
        for x, y, th in _poses(m, fp, r, rng, 500):
            c, s = np.cos(np.float64(th)), np.sin(np.float64(th))
            centre = R.world_to_map(m, x, y)
            if centre is None:
                continue
            n_on_map += 1
            # the largest per-axis offset of a vertex's cell from the centre's (on an unbounded map: the bound is about the
            # arithmetic, not about where the map ends)
            for vx, vy in R.oriented(fp, x, y, c, s):
                for w, o, cc in ((vx, m.origin_x, centre[0]), (vy, m.origin_y, centre[1])):
                    q = R.quotient(w, o, m.resolution)
                    worst = max(worst, abs(math.floor(q) - cc))
            if clear[centre[1], centre[0]]:
                n_clear += 1
                assert R.footprint_code(m, fp, x, y, c, s) == 0, (fname, res, k, x, y, th)
    assert worst <= r, (worst, r)
    assert worst >= r - 2, (worst, r)  # the poses do reach the bound's neighbourhood: ceil(R / res) or one less
    assert n_on_map >= 1000 and n_clear >= 10, (n_on_map, n_clear)
    print(f"{fname} res {res}: r_c {r}, largest offset {worst}, {n_clear} clear of {n_on_map} poses on the map")


def k_seed(fname, res):
    return list(FOOTPRINTS).index(fname) * 10 + RESOLUTIONS.index(res)


def test_window_rule_by_hand():
    """one cost cell: clear exactly where the cell is more than r away on some axis AND the window is on the map"""
    cells = np.zeros((30, 40), dtype=np.uint8)
    cells[12, 17] = 1
    for r in (1, 3, 5):
        clear = CR.clearance_map(cells, r)
        my, mx = np.mgrid[0:30, 0:40]
        inside = (mx >= r) & (mx < 40 - r) & (my >= r) & (my < 30 - r)
        away = (np.abs(mx - 17) > r) | (np.abs(my - 12) > r)
        assert np.array_equal(clear, (inside & away).astype(np.uint8))
    assert not CR.clearance_map(cells, 15).any()  # a window taller than the map is clear nowhere


def test_no_map_for_a_window_of_more_than_129_cells():
    assert CR.half_width([[31.5, 0.0], [-1.0, 0.0], [0.0, 1.0]], 0.5) == 64
    assert CR.half_width([[31.6, 0.0], [-1.0, 0.0], [0.0, 1.0]], 0.5) is None
    assert CR.half_width(np.zeros((0, 2)), 0.05) == 1
