"""The path term (sfw_set_path) restated in numpy: the definition in include/sfw_hip.h, operation by operation and in its
order, vectorised over the poses.  Elementwise float64 operations only, so every product, sum and difference is rounded on
its own as the kernels round it (csrc/sfw_kernels.hip sfw_path_dist_kernel / sfw_path_scan_kernel are compiled without
contraction, csrc/sfw_capi.hip path_segments likewise).

EXACT LAYER, meant to be compared bit for bit: everything here is a fixed sequence of +, -, *, /, compare and select on
float64 — no library function — so given the same poses the device's D and p are these bits."""
from __future__ import annotations

import math

import numpy as np

from ._abi import SFW_PATH_MAX_COORD, SFW_PATH_MAX_POINTS  # noqa: F401  (re-exported)

SFW_COST_INVALID, SFW_COST_SKIPPED = -1.0, -2.0


def check_arguments(xy, weight, reserved=0):
    """what sfw_set_path refuses: ValueError"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    if not 1 <= len(xy) <= SFW_PATH_MAX_POINTS:
        raise ValueError("n_points outside 1 .. SFW_PATH_MAX_POINTS")
    if not np.all(np.abs(xy) <= SFW_PATH_MAX_COORD):  # (a NaN fails the comparison too)
        raise ValueError("a coordinate is not finite or beyond SFW_PATH_MAX_COORD")
    if not math.isfinite(float(weight)):
        raise ValueError("the weight is not finite")
    if reserved != 0:
        raise ValueError("reserved must be 0")


def segment_records(xy):
    """The records {ax, ay, ex, ey, inv} of a path's segments as float64 (n_seg, 5): n - 1 segments of n points, one
    zero-length segment of a single point.  inv = 1 / (ex ex + ey ey), or 0 for a zero-length segment."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    a = xy[:-1] if len(xy) > 1 else xy
    b = xy[1:] if len(xy) > 1 else xy
    ex, ey = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
    len2 = ex * ex + ey * ey
    with np.errstate(divide="ignore"):
        inv = np.where(len2 > 0, 1.0 / len2, 0.0)
    return np.stack([a[:, 0], a[:, 1], ex, ey, inv], axis=1)


def segment_distance(px, py, seg):
    """d of poses (px, py) (arrays) to ONE segment record: the header's five lines"""
    ax, ay, ex, ey, inv = (np.float64(v) for v in seg)
    rx, ry = px - ax, py - ay
    u = (rx * ex + ry * ey) * inv
    t = np.where(u < 0, 0.0, np.where(u > 1, 1.0, u))
    qx, qy = rx - t * ex, ry - t * ey
    return qx * qx + qy * qy


def records_distance(px, py, records):
    """D of poses (px, py) (arrays of one shape) over segment records ((n_seg, 5)): the running minimum `d < m ? d : m` from
    +inf.  A minimum of doubles: the same bits in any segment order."""
    px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    m = np.full(px.shape, np.inf)
    for seg in np.asarray(records, dtype=np.float64).reshape(-1, 5):
        d = segment_distance(px, py, seg)
        m = np.where(d < m, d, m)
    return m


def pose_distance(px, py, path):
    """D of poses (px, py) to the path ((n, 2) points): records_distance over its segment records"""
    return records_distance(px, py, segment_records(path))


def path_term(points, n_points, path):
    """p of every sample.  points: (count, S, 3) Trajectory points (x, y, theta) as sfw_grid_points_batch returns them;
    n_points (nullable): the legal points of each sample — a sample with fewer than S gets SFW_COST_INVALID (the costmap
    rejected it; a caller that knows a sample as skipped puts SFW_COST_SKIPPED there itself).  The sum runs in step order."""
    points = np.asarray(points, dtype=np.float64)
    count, S = points.shape[0], points.shape[1]
    D = pose_distance(points[:, :, 0], points[:, :, 1], path)
    acc = np.zeros(count)
    for i in range(S):
        acc = acc + D[:, i]
    p = acc / np.float64(S)
    if n_points is not None:
        p = np.where(np.asarray(n_points) >= S, p, SFW_COST_INVALID)
    return p


def add(costs, p, w):
    """The cost vector with the term: costs + w * p (a product and a sum, each rounded once) where neither is a sentinel —
    p < 0 is a sample's sentinel, a cost equal to SFW_COST_INVALID a rejection (contact) behind the path pass."""
    costs, p = np.asarray(costs, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return np.where((p >= 0) & (costs != SFW_COST_INVALID), costs + np.float64(w) * p, costs)
