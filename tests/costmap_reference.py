"""The costmap half of a sample's cost in plain Python.  A plain module: no fixtures, nothing pytest collects.

What csrc/sfw_kernels.hip evaluates in three copies (footprint_cost; footprint_edge + k1s_footprint; the list / sequence / batch
instantiations) and oracle/sfw_oracle.cpp in C++, stated once more as nav2's Costmap2D::worldToMap (Foxy),
the reference's LineIterator and its CostmapModel::footprintCost — with the subtraction and division of Python floats and numpy
float64, which ARE the IEEE double operations the reference executes, and Python integers.  No ctypes, no kernel text.  tests/test_costmap_reference.py holds this
module to the oracle and to the recorded reference walks on any machine; tests/test_costmap_edges_gpu.py holds the kernels to it.

The one place where the reference has no defined value: its `(unsigned)(double)` cast of a quotient of 2^32 or more (C++
[conv.fpint]; x86 yields 0 there, the device saturates).  Here such a coordinate is off the map — what both casts give for every
quotient below 2^63 but x86's wrapped values that happen to fall below the size — and the case lists keep to quotients below 2^32
or so far above 2^63 (1e300) that only x86's 0 disagrees; oracle/sfw_oracle.cpp rejects what does not fit an unsigned likewise.

The CASE LISTS of the GPU test live here too (GEOMETRIES, axis_targets, ...), so that the CPU test can hold them to the oracle
and show that they tell cell_index's guarded product from the unguarded one."""
import math
from types import SimpleNamespace as NS

import numpy as np

F64 = np.float64
OFF_MAP, UNKNOWN, LETHAL = -3, -2, -1  # footprint codes below 0, as the reference's footprintCost returns them


# ---- Costmap2D::worldToMap ---------------------------------------------------------------------------------------------------------
def make_map(cells, origin_x, origin_y, resolution):
    cells = np.ascontiguousarray(cells, dtype=np.uint8)
    return NS(cells=cells, size_x=cells.shape[1], size_y=cells.shape[0], origin_x=float(origin_x), origin_y=float(origin_y),
              resolution=float(resolution))


def quotient(w, origin, res):
    """(w - origin) / res as the reference forms it: one IEEE subtraction, one IEEE division (Python floats ARE IEEE doubles,
    and their - and / the same two operations as numpy's, without the cost of numpy scalars; res > 0)"""
    return (float(w) - float(origin)) / float(res)


def axis_cell(w, origin, res, size):
    """The cell of one coordinate, or None: below the origin is rejected first, then the quotient is truncated, then bounded"""
    if float(w) < float(origin):
        return None
    q = quotient(w, origin, res)
    if not q < 4294967296.0:  # (not representable as unsigned, or NaN: see the module docstring)
        return None
    c = int(q)  # truncation; q >= 0 here
    return c if c < size else None


def world_to_map(m, wx, wy):
    """(mx, my) or None.  Both rejections below the origin come first (the reference's one `if`), then each axis"""
    if float(wx) < m.origin_x or float(wy) < m.origin_y:
        return None
    mx, my = axis_cell(wx, m.origin_x, m.resolution, m.size_x), axis_cell(wy, m.origin_y, m.resolution, m.size_y)
    return None if mx is None or my is None else (mx, my)


# ---- cell_index of sfw_kernels.hip, restated for the CPU test alone -----------------------------------------------------------------
def cell_index_product(a, res):
    """trunc(a * fl(1 / res)): what the kernels form first (a >= 0 arrays)"""
    a = np.asarray(a, dtype=F64)
    return np.trunc(a * (F64(1.0) / F64(res)))


def cell_index_guarded(a, res):
    """the kernels' cell_index: the product, and the IEEE division where the product lies within 1e-9 of an integer"""
    a = np.asarray(a, dtype=F64)
    q = a * (F64(1.0) / F64(res))
    m = np.trunc(q)
    d = q - m
    return np.where((d < 1e-9) | (d > 1.0 - 1e-9), np.trunc(a / F64(res)), m)


def cell_index_division(a, res):
    return np.trunc(np.asarray(a, dtype=F64) / F64(res))


# ---- LineIterator ----------------------------------------------------------------------------------------------------------------
def line_cells(x0, y0, x1, y1):
    """The cells the reference's LineIterator visits from (x0, y0) to (x1, y1): max(|dx|, |dy|) + 1 of them, both ends included.
    The longer axis steps every time (x on a tie); the other steps when the running numerator, which starts at half the longer
    extent (integer division) and gains the shorter extent per cell, reaches the longer extent."""
    adx, ady = abs(x1 - x0), abs(y1 - y0)
    sx, sy = (1 if x1 >= x0 else -1), (1 if y1 >= y0 else -1)
    long_is_x = adx >= ady
    den, add = (adx, ady) if long_is_x else (ady, adx)
    num, x, y, out = den // 2, x0, y0, []
    for _ in range(den + 1):
        out.append((x, y))
        num += add
        if num >= den:
            num -= den
            if long_is_x:
                y += sy
            else:
                x += sx
        if long_is_x:
            x += sx
        else:
            y += sy
    return out


# ---- CostmapModel::footprintCost ---------------------------------------------------------------------------------------------------
def oriented(footprint, x, y, c, s):
    """The footprint's vertices in the world for a pose (x, y, cos, sin): x + (qx c - qy s), y + (qx s + qy c), every operation
    an IEEE double one in this order"""
    x, y, c, s = float(x), float(y), float(c), float(s)
    return [(x + (qx * c - qy * s), y + (qx * s + qy * c)) for qx, qy in np.asarray(footprint, dtype=F64).reshape(-1, 2).tolist()]


def line_cost(m, a, b):
    """lineCost: the largest cell on the walk; the first lethal (254) or unknown (255) cell ends it with -1 / -2.  253 is an
    ordinary value on an edge."""
    best = 0
    for x, y in line_cells(a[0], a[1], b[0], b[1]):
        v = int(m.cells[y, x])
        if v == 255:
            return UNKNOWN
        if v == 254:
            return LETHAL
        best = max(best, v)
    return best


def footprint_code(m, footprint, x, y, c, s):
    """The footprint code of a pose: OFF_MAP (-3) for a centre or vertex off the map, UNKNOWN (-2), LETHAL (-1), else 0 .. 253.
    Fewer than three vertices: the centre cell alone, where 253 (inscribed) is lethal too.  Otherwise every edge in order, the
    closing one (last vertex -> first) last, both ends converted before the edge is walked; the first edge that is off the map,
    lethal or unknown decides."""
    centre = world_to_map(m, x, y)
    if centre is None:
        return OFF_MAP
    fp = np.asarray(footprint, dtype=F64).reshape(-1, 2)
    if len(fp) < 3:
        v = int(m.cells[centre[1], centre[0]])
        return UNKNOWN if v == 255 else LETHAL if v in (253, 254) else v
    pts = oriented(fp, x, y, c, s)
    code = 0
    for e in range(len(pts)):
        a, b = pts[e], pts[(e + 1) % len(pts)]
        ca = world_to_map(m, a[0], a[1])
        if ca is None:
            return OFF_MAP
        cb = world_to_map(m, b[0], b[1])
        if cb is None:
            return OFF_MAP
        lc = line_cost(m, ca, cb)
        if lc < 0:
            return lc
        code = max(code, lc)
    return code


def pose_code(m, footprint, x, y, theta):
    """footprint_code at a heading: cos and sin from numpy (exact at 0; elsewhere the device's may differ in the last bit —
    near_edge says where that could matter)"""
    return footprint_code(m, footprint, x, y, np.cos(F64(theta)), np.sin(F64(theta)))


def near_edge(m, footprint, x, y, theta, margin=1e-6):
    """Does any vertex of the pose lie within `margin` (metres) of a cell edge, by this module's own numbers?  (The centre does
    not pass through cos and sin: it is never in doubt.)"""
    if len(footprint) < 3:
        return False
    for px, py in oriented(footprint, x, y, np.cos(F64(theta)), np.sin(F64(theta))):
        for w, o in ((px, m.origin_x), (py, m.origin_y)):
            q = float(quotient(w, o, m.resolution))
            if math.isfinite(q) and abs(q - round(q)) * m.resolution < margin:
                return True
    return False


def in_doubt(m, footprint, x, y, theta):
    """Is the pose left out of a comparison with the device?  Only where the device's cos and sin may differ from numpy's in a
    way that matters: not at heading 0 (1 and 0 exactly), and not at the double pi/2 — there sin is exactly 1 (the address
    launches of tests/test_costmap_edges_gpu.py assert it: their pose 1 is start + 0.25 v on the y axis, bit for bit) and cos is
    6.1e-17, whose last bit (1e-32) could show in qx cos - qy sin only at an exact rounding tie — so the sweeps along y at
    heading pi/2 put vertices ON edge coordinates like those along x.  Anywhere else: near_edge."""
    return theta != 0.0 and theta != math.pi / 2 and near_edge(m, footprint, x, y, theta)


# ---- a sample's verdict ------------------------------------------------------------------------------------------------------------
def verdict(codes):
    """(rejected, n_points, costmap term) of a sample from its poses' codes in step order: the first illegal step (a code below 0,
    or 254 / 255) rejects — n_points is the number of legal poses in front of it; otherwise the term is
    (sum in step order of code / 255.0) / S, each a double operation (oracle/sfw_oracle.cpp:375-381; SFW_TERM_COSTMAP)"""
    cm = F64(0.0)
    for i, code in enumerate(codes):
        if code < 0 or code >= 254:
            return True, i, None
        cm = cm + F64(code) / F64(255.0)
    return False, len(codes), float(cm / F64(len(codes)))


# ---- the case lists ----------------------------------------------------------------------------------------------------------------
THIRD = 1.0 / 3.0
FAR = 1e4 + 0.05  # odometry far from zero
# name -> (size_x, size_y, origin_x, origin_y, resolution).  "wide": size_x > size_y, "tall": the reverse.  Every resolution and
# every origin of the issue appears on an x axis and on a y axis; origin_x != origin_y everywhere.
GEOMETRIES = {
    "wide_37x23_r0.05": (37, 23, 0.0, -0.85, 0.05),
    "tall_23x37_r0.1": (23, 37, -0.85, 0.0, 0.1),
    "wide_250x3_r0.025": (250, 3, 1.7, -0.0375, 0.025),
    "tall_3x250_r0.03": (3, 250, -0.045, 1.7, 0.03),
    "wide_64x1_r0.07": (64, 1, FAR, -0.035, 0.07),
    "tall_1x64_r0.333": (1, 64, -0.85, FAR, THIRD),
    "wide_37x23_r0.333": (37, 23, 1.7, 0.0, THIRD),
    "tall_23x37_r0.07": (23, 37, 0.0, FAR, 0.07),
    "wide_37x23_r0.03": (37, 23, FAR, 1.7, 0.03),
    "tall_23x37_r0.025": (23, 37, -0.85, 1.7, 0.025),
    "wide_37x23_r0.1": (37, 23, -0.85, FAR, 0.1),
    "tall_23x37_r0.05": (23, 37, 1.7, -0.85, 0.05),
    "wide_37x23_r0.5": (37, 23, -0.85, 0.0, 0.5),
    "tall_23x37_r4": (23, 37, 0.0, -0.85, 4.0),
}


def geometry(name):
    sx, sy, ox, oy, res = GEOMETRIES[name]
    return NS(name=name, size_x=sx, size_y=sy, origin_x=ox, origin_y=oy, resolution=res)


def address_map(g, axis):
    """cells[my, mx] = mx (axis 0) or my (axis 1): with both sizes below 253 and a point footprint the code IS the cell index"""
    assert g.size_x < 253 and g.size_y < 253
    my, mx = np.mgrid[0:g.size_y, 0:g.size_x]
    return make_map((mx if axis == 0 else my).astype(np.uint8), g.origin_x, g.origin_y, g.resolution)


def _neighbours(v):
    v = F64(v)
    return [np.nextafter(v, F64(-np.inf)), v, np.nextafter(v, F64(np.inf))]


def axis_targets(origin, res, size):
    """The coordinates one axis is probed at: every origin + k res for k = 0 .. size with its two neighbouring doubles (k = 0
    gives nextafter(origin, -inf)), -0.0, +-1e6 and +-1e300"""
    out = []
    for k in range(size + 1):
        out += _neighbours(F64(origin) + F64(k) * F64(res))
    out += [F64(-0.0), F64(1e6), F64(-1e6), F64(1e300), F64(-1e300)]
    return np.array(out, dtype=F64)


def mid_cell(origin, res, size):
    """a coordinate well inside a cell in the middle of the axis"""
    return float(F64(origin) + (F64(size // 2) + F64(0.5)) * F64(res))


def axis_start(origin, res, size):
    """Where the robot stands on the probed axis: at 0.0 where the map contains it (pose 1 = 0 + 0.25 v is then exactly the
    target), else at the origin itself"""
    return 0.0 if origin <= 0.0 < origin + size * res else float(origin)


DT = 0.25  # the power-of-two step of every multi-pose launch


def axis_commands(origin, res, size):
    """(start, velocities, pose-1 coordinates): the velocity that takes the robot from `start` to each target in one step of DT
    with unlimited acceleration, and where start + DT v lands in IEEE arithmetic — the coordinates the check really sees (the
    targets themselves from start 0.0; within an ulp of them otherwise, and still with both neighbours)"""
    start = axis_start(origin, res, size)
    t = axis_targets(origin, res, size)
    with np.errstate(over="ignore"):
        v = (t - F64(start)) / F64(DT)
        v = v[np.isfinite(v)]
        landed = F64(start) + v * F64(DT)
    return start, v, landed


def step0_targets(origin, res, size):
    """coordinates handed over as the robot's own pose (step 0 is untouched): what no velocity reaches from the start"""
    return np.array([F64(-0.0), np.nextafter(F64(origin), F64(-np.inf)), F64(origin), np.nextafter(F64(origin) + F64(size) * F64(res), F64(-np.inf)),
                     F64(origin) + F64(size) * F64(res), F64(1e6), F64(-1e6), F64(1e300), F64(-1e300)], dtype=F64)


# -- footprints
BOX = [[0.4, 0.3], [-0.4, 0.3], [-0.4, -0.3], [0.4, -0.3]]  # synthetic.make_footprint("box")
TRIANGLE = [[0.3, 0.0], [-0.2, 0.25], [-0.2, -0.15]]
SLIVER = [[0.001, 0.0], [-0.001, 0.001], [-0.001, -0.001]]  # K = 3, every vertex in the centre's cell


def polygon16(radius=0.35):
    """synthetic.make_footprint("polygon16")"""
    a = np.arange(16) * (2.0 * math.pi / 16)
    return np.stack([radius * np.cos(a), radius * np.sin(a)], axis=1).astype(F64)


OFFSET_TRIANGLE = [[0.1, 0.0], [0.3, 0.1], [0.3, -0.1]]  # does not contain its centre: the centre can be off the map alone


def random_map(g, seed, clear_xy, clear_radius=0.6):
    """a random map of ordinary values with a few 253 / 254 / 255 cells, none of them within clear_radius of clear_xy (where
    the robot starts: a start that is illegal hides every later pose)"""
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, 253, (g.size_y, g.size_x)).astype(np.uint8)
    n = max(g.size_x * g.size_y // 150, 1)
    my, mx = np.mgrid[0:g.size_y, 0:g.size_x]
    cx, cy = g.origin_x + (mx + 0.5) * g.resolution, g.origin_y + (my + 0.5) * g.resolution
    far = np.hypot(cx - clear_xy[0], cy - clear_xy[1]) > clear_radius + g.resolution
    for v in (253, 254, 255):
        ys, xs = rng.integers(0, g.size_y, n), rng.integers(0, g.size_x, n)
        keep = far[ys, xs]
        cells[ys[keep], xs[keep]] = v
    return make_map(cells, g.origin_x, g.origin_y, g.resolution)


# -- segments (cell coordinates relative to the first end): all eight octants, |dx| == |dy|, horizontal, vertical, one cell
SEGMENTS = [(7, 3), (3, 7), (-3, 7), (-7, 3), (-7, -3), (-3, -7), (3, -7), (7, -3), (5, 5), (-5, 5), (-5, -5), (5, -5),
            (6, 0), (-6, 0), (0, 6), (0, -6), (0, 0), (1, 0), (0, 1), (8, 1), (1, 8), (-8, 5), (4, -2)]


def segment_footprint(dx, dy, res):
    """A K = 3 footprint whose first edge runs from the centre's cell to the cell (dx, dy) away: vertices at the centre, the far
    cell's centre, and the far cell's centre again (edge 1 stays in that cell; the closing edge walks back)"""
    far = [dx * res, dy * res]
    return [[0.0, 0.0], far, far]


# ---- launches: what the GPU test runs through every kernel path, and the CPU test through the oracle --------------------------------
ACC = 1e308  # acceleration limits under which every velocity reaches its sample in the first step
POLY_GEOMETRIES = ["wide_37x23_r0.333", "tall_23x37_r0.1", "tall_23x37_r0.07"]
RANDOM_CASES = [("wide_120x80_r0.05", "polygon16", 7), ("tall_80x120_r0.07", "box", 8)]  # (geometry, footprint, seed)
GEOMETRIES["wide_120x80_r0.05"] = (120, 80, -2.3, -1.9, 0.05)
GEOMETRIES["tall_80x120_r0.07"] = (80, 120, 1.7, FAR, 0.07)
FOOTPRINTS = {"point": np.zeros((0, 2)), "box": np.array(BOX), "polygon16": polygon16(), "triangle": np.array(TRIANGLE),
              "sliver": np.array(SLIVER), "offset_triangle": np.array(OFFSET_TRIANGLE)}
HALF_PI = math.pi / 2


def spec(name, m, footprint, start, lin, ang=(0.0,), S=2, vy=None, **extra):
    """One launch: the robot at `start` (x, y, theta) at rest, the grid lin x ang (or, with vy, the list (lin[t], vy[t], 0) —
    holonomic, so a list or a sequence only), S steps of DT.  The way-point is the start."""
    x, y, th = (float(v) for v in start)
    return NS(name=name, map=m, footprint=np.asarray(footprint, dtype=F64).reshape(-1, 2), rs=(x, y, th, 0.0, 0.0, 0.0),
              goal=(ACC, ACC, ACC, x if math.isfinite(x) and abs(x) < 1e5 else 0.0, y if math.isfinite(y) and abs(y) < 1e5 else 0.0),
              lin=np.asarray(lin, dtype=F64), ang=np.asarray(ang, dtype=F64), S=S, vy=None if vy is None else np.asarray(vy, dtype=F64),
              **extra)


def samples(sp, ang=None):
    """(vx, vy, vtheta) of every sample of a launch in sample order (grid: t = iv * nw + iw)"""
    if sp.vy is not None:
        return sp.lin.copy(), sp.vy.copy(), np.zeros(len(sp.lin))
    ang = sp.ang if ang is None else np.asarray(ang, dtype=F64)
    return np.repeat(sp.lin, len(ang)), np.zeros(len(sp.lin) * len(ang)), np.tile(ang, len(sp.lin))


def rollout(rs, vx, vy, vth, S):
    """The poses the footprint is checked at, (n, S, 3): the pose BEFORE each step; the velocities are the samples from the first
    step on (ACC); x and y advance with the OLD heading (oracle/sfw_oracle.cpp:384-391)"""
    n = len(vx)
    x, y, th = np.full(n, F64(rs[0])), np.full(n, F64(rs[1])), np.full(n, F64(rs[2]))
    out = np.zeros((n, S, 3))
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(S):
            out[:, i, 0], out[:, i, 1], out[:, i, 2] = x, y, th
            xn = x + (vx * np.cos(th) + vy * np.cos(HALF_PI + th)) * DT
            yn = y + (vx * np.sin(th) + vy * np.sin(HALF_PI + th)) * DT
            x, y, th = xn, yn, th + vth * DT
    return out


def expected(sp, poses, tally=None):
    """Per sample of poses (n, S, 3): (rejected, n_points, costmap term), or None for a sample that is left out because a pose
    that matters has a heading other than 0 and a vertex within 1e-6 of a cell edge.  tally (a dict) counts the poses looked at
    and the poses left out."""
    cache, out = {}, []
    for traj in poses:
        codes, left_out = [], False
        for x, y, th in traj:
            key = (float(x).hex(), float(y).hex(), float(th).hex())
            if key not in cache:
                skip = in_doubt(sp.map, sp.footprint, x, y, th)
                cache[key] = (None if skip else pose_code(sp.map, sp.footprint, x, y, th))
                if tally is not None:
                    tally["poses"] = tally.get("poses", 0) + 1
                    tally["left_out"] = tally.get("left_out", 0) + (1 if skip else 0)
            code = cache[key]
            if code is None:
                left_out = True
                break
            codes.append(code)
            if code < 0 or code >= 254:
                break
        out.append(None if left_out else verdict(codes))  # (codes: every pose, or up to the first illegal one)
    return out


def _mid(g):
    return mid_cell(g.origin_x, g.resolution, g.size_x), mid_cell(g.origin_y, g.resolution, g.size_y)


def address_specs(gname):
    """Point footprint on the two address maps: per axis, every edge coordinate of axis_targets at pose 1 (x: heading 0; y:
    heading pi/2), then step0_targets as the handed-over pose itself"""
    g = geometry(gname)
    mx, my = _mid(g)
    out = []
    for axis, (o, size) in enumerate(((g.origin_x, g.size_x), (g.origin_y, g.size_y))):
        start, v, landed = axis_commands(o, g.resolution, size)
        pose = (start, my, 0.0) if axis == 0 else (mx, start, HALF_PI)
        for addr in (0, 1):
            out.append(spec(f"{gname} axis {axis} map {addr}", address_map(g, addr), FOOTPRINTS["point"], pose, v, axis=axis, landed=landed))
        for w in step0_targets(o, g.resolution, size):
            pose = (w, my, 0.0) if axis == 0 else (mx, w, HALF_PI)
            out.append(spec(f"{gname} axis {axis} step 0 at {float(w)!r}", address_map(g, axis), FOOTPRINTS["point"], pose,
                            [g.resolution, 2.0 * g.resolution], axis=axis, landed=None))
    return out


def polygon_specs(gname):
    """Every polygon over a random map, swept along x (heading 0) and along y (heading pi/2 for a grid; holonomic at heading 0
    for a list) so that a vertex — the first, and the one with the smallest coordinate — meets every edge coordinate of
    axis_targets: both borders are straddled, the last row and column touched exactly, the centre leaves the map before or
    after the vertices"""
    g = geometry(gname)
    mx, my = _mid(g)
    out = []
    for k, (fname, fp) in enumerate(FOOTPRINTS.items()):
        if fname == "point":
            continue
        m = random_map(g, 100 + k, (mx, my))
        for vtx in sorted({0, int(np.argmin(fp[:, 0]))}):
            qx = float(fp[vtx, 0])
            tx = axis_targets(g.origin_x, g.resolution, g.size_x) - qx
            ty = axis_targets(g.origin_y, g.resolution, g.size_y) - qx  # (heading pi/2: the vertex's world y is y + qx)
            with np.errstate(over="ignore"):
                vx, vyg = (tx - mx) / DT, (ty - my) / DT
            out.append(spec(f"{gname} {fname} vertex {vtx} along x", m, fp, (mx, my, 0.0), vx[np.isfinite(vx)]))
            out.append(spec(f"{gname} {fname} vertex {vtx} along y, heading pi/2", m, fp, (mx, my, HALF_PI), vyg[np.isfinite(vyg)]))
        for vtx in sorted({0, int(np.argmin(fp[:, 1]))}):
            ty = axis_targets(g.origin_y, g.resolution, g.size_y) - float(fp[vtx, 1])
            with np.errstate(over="ignore"):
                vy = (ty - my) / DT
            vy = vy[np.isfinite(vy)]
            out.append(spec(f"{gname} {fname} vertex {vtx} along y, holonomic", m, fp, (mx, my, 0.0), np.zeros(len(vy)), vy=vy))
    return out


def random_specs():
    """~2000 poses with random headings per case: S = 3, poses 1 and 2 of a 32 x 32 grid"""
    out = []
    for gname, fname, seed in RANDOM_CASES:
        g = geometry(gname)
        mx, my = _mid(g)
        rng = np.random.default_rng(seed)
        out.append(spec(f"random headings {gname} {fname}", random_map(g, seed, (mx, my)), FOOTPRINTS[fname], (mx, my, 0.3),
                        rng.uniform(-3.0, 3.0, 32), rng.uniform(-8.0, 8.0, 32), S=3))
    return out


SEG_GEOMETRY = NS(name="segments", size_x=64, size_y=44, origin_x=-3.25, origin_y=1.75, resolution=0.5)
SEG_START, SEG_MARK = (10, 22), (40, 22)  # cells: the robot's, and the column / pose row of the marked cell


def segment_cells(dx, dy):
    """(cells on the footprint of segment_footprint relative to the centre's cell, cells next to them but not on it)"""
    on = set(line_cells(0, 0, dx, dy)) | set(line_cells(dx, dy, dx, dy)) | set(line_cells(dx, dy, 0, 0))
    beside = {(x + i, y + j) for x, y in on for i in (-1, 0, 1) for j in (-1, 0, 1)} - on
    return on, beside


def segment_specs(segments=None):
    """Per segment and per row of cells it or its neighbours touch: a zero map with ONE cell of 200, and one sample per cell of
    that row — on the footprint or next to it — whose pose 1 puts that cell of the footprint on the marked one.  Cell centres at
    a resolution of 0.5: every coordinate is exact.  sp.hits[t]: is sample t's cell on the footprint?"""
    g = SEG_GEOMETRY
    centre = lambda c, o: o + (c + 0.5) * g.resolution  # noqa: E731
    x0, y0 = centre(SEG_START[0], g.origin_x), centre(SEG_START[1], g.origin_y)
    out = []
    for dx, dy in (SEGMENTS if segments is None else segments):
        on, beside = segment_cells(dx, dy)
        for row in sorted({y for _, y in on | beside}):
            cols = sorted(x for x, y in on | beside if y == row)
            cells = np.zeros((g.size_y, g.size_x), dtype=np.uint8)
            cells[SEG_MARK[1] + row, SEG_MARK[0]] = 200
            lin = [(centre(SEG_MARK[0] - c, g.origin_x) - x0) / DT for c in cols]
            out.append(spec(f"segment {(dx, dy)} row {row}", make_map(cells, g.origin_x, g.origin_y, g.resolution),
                            segment_footprint(dx, dy, g.resolution), (x0, y0, 0.0), lin, hits=[(c, row) in on for c in cols]))
    return out


def illegal_specs():
    """The illegal-value classes: 252 .. 255 under a point footprint; 253, 254, 255 on a box's edge; a lethal wall that samples
    of different speeds reach at different steps (point and box)"""
    out = []
    g = geometry("wide_37x23_r0.05")
    mx, my = _mid(g)
    row = int((my - g.origin_y) / g.resolution)
    cells = np.zeros((g.size_y, g.size_x), dtype=np.uint8)
    for col, v in ((24, 252), (26, 253), (28, 254), (30, 255)):
        cells[row, col] = v
    lin = [(g.origin_x + (c + 0.5) * g.resolution - mx) / DT for c in range(20, 34)]
    out.append(spec("point on 252 .. 255", make_map(cells, g.origin_x, g.origin_y, g.resolution), FOOTPRINTS["point"], (mx, my, 0.0), lin))
    g = geometry("wide_120x80_r0.05")
    mx, my = _mid(g)
    edge_row = int((my + 0.3 - g.origin_y) / g.resolution)  # the row of the box's upper edge
    lin = [(g.origin_x + (c + 0.5) * g.resolution - mx) / DT for c in range(60, 110, 2)]
    for v in (253, 254, 255):
        cells = np.zeros((g.size_y, g.size_x), dtype=np.uint8)
        cells[edge_row, 90] = v
        out.append(spec(f"box with {v} on an edge", make_map(cells, g.origin_x, g.origin_y, g.resolution), FOOTPRINTS["box"], (mx, my, 0.0), lin))
    cells = np.full((g.size_y, g.size_x), 7, dtype=np.uint8)
    cells[:, 100] = 254
    wall = g.origin_x + 100.5 * g.resolution - mx
    lin = [wall / (j * DT) * f for j in (1, 2, 3, 4) for f in (0.7, 1.0)] + [0.1, -0.2]
    for fname in ("point", "box"):
        out.append(spec(f"a wall behind legal steps, {fname}", make_map(cells, g.origin_x, g.origin_y, g.resolution), FOOTPRINTS[fname],
                        (mx, my, 0.0), lin, S=5))
    return out
