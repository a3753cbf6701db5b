"""The costmap half of a sample's cost — worldToMap, the footprint check, the costmap term — against tests/costmap_reference.py,
bit for bit, off the square 0.05 m map every other GPU test uses: non-square maps and strips, eight resolutions, origins that
differ per axis, a map that does not contain the world origin, odometry at 1e4, and coordinates ON cell edges with both
neighbouring doubles — where cell_index (sfw_kernels.hip) must take the IEEE division and tests/test_costmap_reference.py shows
that its reciprocal product alone would be wrong.

Everything compared is an integer decision or a fixed IEEE sequence applied to one: cost sentinels, point counts,
SFW_TERM_COSTMAP and Trajectory points are asserted BIT FOR BIT, no tolerance anywhere.

How an exact pose gets into the check (costmap_reference.spec): the footprint is tested at the pose before each step; step 0 is
the handed-over pose; from a robot at rest with unlimited acceleration pose 1 is start + 0.25 v, exact for a start of 0.0 and
within an ulp of the target otherwise (the target's neighbours are targets too).  Whatever the launch, the device's OWN poses are
read back (sfw_grid_points_batch returns every pose, legal or not) and fed to the reference, so the check isolates the footprint
from the rollout; where a launch is meant to hit given coordinates the poses are asserted to be those coordinates.  A pose with a
heading other than 0 goes through the device's sincos, which may differ from numpy's in the last bit: a sample is left out when
such a pose has a vertex within 1e-6 m of a cell edge by the reference's own numbers (the random-heading launches may leave out
1 % at most; they leave out 2 poses of 2518 in one launch and none in the others).

Every family of launches runs through every kernel path — plan_info() says which one ran:
    cycle       the one-launch cycle kernel (a grid of at most 1024 samples)
    small       sfw_rollout_small_kernel (SFW_CYCLE_FUSED=0)
    k1abc       K1a + K1b + K1c: a grid of more than 2048 samples, no people
    list, list_small, list_k1abc   the same three for a sample list (the LIST instantiations read cs_tab / ptab at other strides)
    sequence    two knots: the SEQ instantiation, one more step, the second knot the samples in reverse order
    batch       one sfw_batch launch of three members with different map geometries
Mutations of the kernels that these tests were seen to catch: profiles/r21_costmap_edges.txt."""
import numpy as np
import pytest

import costmap_reference as R
from sfw_test_util import _bits, _same
from social_force_window_planner_amd._abi import SFW_TERM_COSTMAP, SfwAgent, default_params

pytestmark = pytest.mark.gpu

GRID_PATHS = ["cycle", "small", "k1abc"]
LIST_PATHS = ["list", "list_small", "list_k1abc", "sequence"]
PATHS = GRID_PATHS + LIST_PATHS
AXIS_GEOMETRIES = list(R.GEOMETRIES)


def _params(S):
    return default_params(sim_time=S * R.DT, sim_granularity=R.DT)


def _load(g, sp, S):
    g.set_params(_params(S))
    g.set_costmap(sp.map.cells, sp.map.origin_x, sp.map.origin_y, sp.map.resolution)
    g.set_footprint(sp.footprint)
    g.set_agents((SfwAgent * 0)())
    g.set_terms_capture(True)


def _wide_ang(sp):
    """the grid's angular velocities extended (by values other than its own) until the grid has more than 2048 samples"""
    nw = max(-(-2049 // len(sp.lin)), len(sp.ang))
    return np.concatenate([sp.ang, 0.01 * (1 + np.arange(nw - len(sp.ang)))])


def _read(g, sp, S, costs, vx, vy, vth, grid):
    T = len(costs)
    pts, n = g.grid_points_batch(0, T, S)
    skipped = (vx == 0.0) & (vth == 0.0) if grid else np.zeros(T, dtype=bool)
    per = 1 if sp.vy is not None else (T // len(sp.lin) if grid else len(sp.ang))  # consecutive samples per entry of sp.lin
    iv = np.resize(np.repeat(np.arange(len(sp.lin)), per), T)  # (a tiled list goes round again)
    assert np.array_equal(sp.lin[iv], vx)  # iv: which entry of sp.lin (of sp.landed, sp.hits) a sample is
    return R.NS(spec=sp, S=S, costs=np.array(costs), cm=g.cost_terms()[:, SFW_TERM_COSTMAP].copy(), pts=pts, n=n, skipped=skipped,
                vx=vx, vy=vy, vth=vth, iv=iv)


def _launch(g, monkeypatch, path, sp):
    """one launch of `sp` on handle g through `path`"""
    monkeypatch.setenv("SFW_CYCLE_FUSED", "0" if path in ("small", "list_small") else "1")
    S = sp.S + 1 if path == "sequence" else sp.S
    _load(g, sp, S)
    if path in GRID_PATHS:
        assert sp.vy is None
        ang = _wide_ang(sp) if path == "k1abc" else sp.ang
        costs, _ = g.score_grid(sp.rs, sp.lin, ang, sp.goal)
        vx, vy, vth = R.samples(sp, ang)
        out = _read(g, sp, S, costs, vx, vy, vth, True)
    else:
        vx, vy, vth = R.samples(sp)
        if path == "list_k1abc":
            k = -(-2049 // len(vx))
            vx, vy, vth = np.tile(vx, k), np.tile(vy, k), np.tile(vth, k)
        if path == "sequence":
            costs, _ = g.score_sequences(sp.rs, np.stack([vx, vx[::-1]]), np.stack([vth, vth[::-1]]), (0, 1), sp.goal, vy=np.stack([vy, vy[::-1]]))
        else:
            costs, _ = g.score_samples(sp.rs, vx, vth, sp.goal, vy=vy)
        out = _read(g, sp, S, costs, vx, vy, vth, False)
    info = g.plan_info()
    assert info["samples"] == len(out.costs)
    if path in ("cycle", "list", "sequence"):
        assert info["one_launch"] == 1, info
    elif path in ("small", "list_small"):
        assert info["one_launch"] == 0 and info["samples"] <= 2048, info
    else:
        assert info["one_launch"] == 0 and info["samples"] > 2048 and info["chunks"] == 1, info
    return out


def _check(out, tally=None, thin=False):
    """every sample of a launch against the reference's verdict on the device's own poses.  thin: of the samples whose poses
    have headings other than 0 only every seventh (a launch widened to 2048 samples with a polygon: the reference is Python)"""
    sp = out.spec
    T, S = len(out.costs), out.S
    assert out.pts.shape == (T, S, 3)
    start = np.array(sp.rs[:3])
    assert np.array_equal(_bits(out.pts[~out.skipped, 0]), np.broadcast_to(_bits(start), (int((~out.skipped).sum()), 3))), sp.name
    pick = np.flatnonzero(~out.skipped)
    if thin:
        level = np.all(out.pts[pick, :, 2] == 0.0, axis=1)
        pick = np.concatenate([pick[level], pick[~level][::7]])
    want = R.expected(R.NS(map=sp.map, footprint=sp.footprint), out.pts[pick], tally)
    bad, checked = [], 0
    for t, w in zip(pick.tolist(), want):
        if w is None:
            continue
        checked += 1
        rejected, n_points, cm = w
        got = (float(out.costs[t]), int(out.n[t]), float(out.cm[t]).hex())
        ok = got[1] == n_points and ((got[0] == -1.0 and out.cm[t] == -1.0) if rejected else (got[0] >= 0.0 and got[2] == float(cm).hex()))
        if not ok:
            bad.append((t, out.pts[t].tolist(), got, (rejected, n_points, None if cm is None else float(cm).hex())))
    assert not bad, (sp.name, len(bad), bad[:3])
    assert np.all(out.costs[out.skipped] == -2.0) and np.all(out.n[out.skipped] == 0)
    assert checked > 0
    # heading 0 throughout and no lateral velocity: every pose is x + 0.25 v exactly, numpy's rollout IS the device's
    if sp.rs[2] == 0.0 and not np.any(out.vth) and not np.any(out.vy) and S == sp.S:
        assert _same(out.pts[~out.skipped], R.rollout(sp.rs, out.vx, out.vy, out.vth, S)[~out.skipped]), sp.name
    return checked


def _check_landed(out):
    """an address launch's pose 1 is, on the probed axis, the coordinate the case list says (costmap_reference.axis_commands)"""
    sp = out.spec
    if sp.landed is None:
        return
    got, want = out.pts[:, 1, sp.axis], sp.landed[out.iv]
    assert np.array_equal(_bits(got[~out.skipped]), _bits(want[~out.skipped])), sp.name


def _no_holonomic(path, specs):
    return [sp for sp in specs if sp.vy is None or path in LIST_PATHS]


# ---- the families, through every path of one handle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", AXIS_GEOMETRIES)
@pytest.mark.parametrize("path", PATHS)
def test_address_maps(hip_mod, monkeypatch, path, gname):
    """point footprint, cells[my, mx] = mx and = my: the costmap term IS the cell index of every edge coordinate"""
    g = hip_mod.HipScorer(_params(2))
    for sp in R.address_specs(gname):
        out = _launch(g, monkeypatch, path, sp)
        _check(out)
        if path != "sequence":
            _check_landed(out)
    g.close()


@pytest.mark.parametrize("gname", R.POLY_GEOMETRIES)
@pytest.mark.parametrize("path", PATHS)
def test_polygons(hip_mod, monkeypatch, path, gname):
    """box, polygon16, a triangle, a sliver inside one cell, a triangle beside its centre: vertices on every edge coordinate, all
    four borders straddled"""
    g = hip_mod.HipScorer(_params(2))
    for sp in _no_holonomic(path, R.polygon_specs(gname)):
        _check(_launch(g, monkeypatch, path, sp), thin=path == "k1abc")
    g.close()


@pytest.mark.parametrize("path", PATHS)
def test_random_headings(hip_mod, monkeypatch, path):
    g = hip_mod.HipScorer(_params(3))
    for sp in R.random_specs():
        tally = {}
        checked = _check(_launch(g, monkeypatch, path, sp), tally)
        print(f"{path}: {sp.name}: {tally['left_out']} of {tally['poses']} poses left out, {checked} samples checked")
        assert tally["left_out"] <= 0.01 * tally["poses"] and tally["poses"] >= 1500, tally
    g.close()


@pytest.mark.parametrize("path", PATHS)
def test_segments(hip_mod, monkeypatch, path):
    """the device's walk against the reference's cell list, cell by cell: the one marked cell is seen exactly from the poses that
    put a cell of the walk on it, never from a neighbouring one"""
    g = hip_mod.HipScorer(_params(2))
    hit, miss = float(np.float64(200.0) / 255.0 / 2), 0.0  # (0 / 255 + 200 / 255) / 2: pose 0 sees no marked cell
    for sp in R.segment_specs():
        out = _launch(g, monkeypatch, path, sp)
        _check(out, thin=path == "k1abc")
        if path != "sequence":  # (a sequence has a third pose)
            level = out.pts[:, 1, 2] == 0.0
            assert np.array_equal(out.cm[level], np.where(np.array(sp.hits)[out.iv], hit, miss)[level]), sp.name
    g.close()


@pytest.mark.parametrize("path", PATHS)
def test_illegal_value_classes(hip_mod, monkeypatch, path):
    g = hip_mod.HipScorer(_params(2))
    seen = set()
    for sp in R.illegal_specs():
        out = _launch(g, monkeypatch, path, sp)
        _check(out)
        seen |= {int(n) for n, c in zip(out.n, out.costs) if c == -1.0}
    assert {1, 2, 3, 4} <= seen  # rejected behind 1 .. 4 legal poses
    g.close()


# ---- one batch launch of members with different geometries -----------------------------------------------------------------------------
def _batch(hip_mod, monkeypatch, members):
    monkeypatch.setenv("SFW_CYCLE_FUSED", "1")
    bs = hip_mod.BatchScorer(_params(2), 0, len(members))
    for i, sp in enumerate(members):
        _load(bs.member(i), sp, sp.S)
        bs.stage(i, sp.rs, sp.lin, sp.ang, sp.goal)
    bs.launch()
    bs.fetch()
    assert bs.describe()["one_launch_members"] == len(members)
    outs = []
    for i, sp in enumerate(members):
        h = bs.member(i)
        outs.append(_read(h, sp, sp.S, h.costs_view().copy(), *R.samples(sp), True))
    bs.close()
    return outs


def _in_threes(lists):
    """members of one launch from three different lists, as long as all three last"""
    return [list(m) for m in zip(*lists)]


@pytest.mark.parametrize("first", range(0, len(AXIS_GEOMETRIES) - 2, 3))
def test_batch_address_maps(hip_mod, monkeypatch, first):
    names = AXIS_GEOMETRIES[first:first + 3]
    for members in _in_threes([R.address_specs(n) for n in names]):
        assert len({(m.map.size_x, m.map.size_y, m.map.origin_x, m.map.origin_y, m.map.resolution) for m in members}) == 3
        for out in _batch(hip_mod, monkeypatch, members):
            _check(out)
            _check_landed(out)


def test_batch_polygons_random_headings_segments_and_illegal_values(hip_mod, monkeypatch):
    poly = [_no_holonomic("batch", R.polygon_specs(n)) for n in R.POLY_GEOMETRIES]
    seg, ill = R.segment_specs([(7, 3), (-3, -7), (5, 5)]), R.illegal_specs()
    launches = _in_threes(poly) + [R.random_specs() + [poly[0][0]]] + [seg[i:i + 4] for i in range(0, len(seg), 4)] + [ill[:4], ill[3:]]
    for members in launches:
        for out in _batch(hip_mod, monkeypatch, members):
            _check(out)


# ---- map changes on one handle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["cycle", "small", "k1abc", "list"])
def test_map_changes_on_one_handle(hip_mod, monkeypatch, path):
    """the rolling local costmap of a controller: the same bytes under a moved origin, the same byte count with size_x and
    size_y exchanged, larger, smaller and larger maps — after every change the handle scores as a fresh one does"""
    a = R.address_specs("wide_37x23_r0.05")[0]
    big, strip = R.address_specs("wide_120x80_r0.05"), R.address_specs("tall_3x250_r0.03")

    def on(sp, m):
        return R.NS(**{**vars(sp), "map": m, "landed": None})
    moved = on(a, R.make_map(a.map.cells, a.map.origin_x - 0.1, a.map.origin_y + 0.1, a.map.resolution))
    turned = on(a, R.make_map(a.map.cells.reshape(a.map.size_x, a.map.size_y), a.map.origin_x, a.map.origin_y, a.map.resolution))
    assert turned.map.cells.tobytes() == a.map.cells.tobytes() and (turned.map.size_x, turned.map.size_y) == (a.map.size_y, a.map.size_x)
    g = hip_mod.HipScorer(_params(2))
    results = []
    for sp in (a, moved, a, turned, big[0], strip[0], big[1], a, turned, moved):
        out = _launch(g, monkeypatch, path, sp)
        _check(out)
        fresh = hip_mod.HipScorer(_params(2))
        ref = _launch(fresh, monkeypatch, path, sp)
        fresh.close()
        assert _same(out.costs, ref.costs) and _same(out.cm, ref.cm) and _same(out.pts, ref.pts) and np.array_equal(out.n, ref.n), sp.name
        results.append(out.cm)
    assert not _same(results[0], results[1]) and not _same(results[0], results[3])  # the changes matter
    g.close()
