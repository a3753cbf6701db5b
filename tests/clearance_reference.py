"""The footprint check's clearance map in numpy.  A plain module: no fixtures, nothing pytest collects.

clear[c] = 1 exactly when every cell of the square window of half-width r_c around cell c lies on the map and has cost 0
(csrc/sfw_kernels.hip sfw_clearance_rows_kernel / sfw_clearance_cols_kernel); r_c = ceil(R / res) + 1 with R the largest vertex
distance of the footprint (csrc/sfw_capi.hip clearance_half_width), and no map at all when r_c exceeds MAX_HALF_WIDTH.
tests/test_footprint_clearance.py holds the rule to tests/costmap_reference.py on any machine;
tests/test_footprint_clearance_gpu.py holds the kernels to this module."""
import math

import numpy as np

MAX_HALF_WIDTH = 64  # SFW_CLEAR_MAX_HALF_WIDTH: a window of at most 129 cells


def half_width(footprint, res):
    """r_c of a footprint ((K, 2), K >= 0) at a resolution, or None when the window would be wider than 129 cells"""
    fp = np.asarray(footprint, dtype=np.float64).reshape(-1, 2)
    R = max((math.hypot(x, y) for x, y in fp.tolist()), default=0.0)
    q = math.ceil(R / float(res)) + 1
    return int(q) if q <= MAX_HALF_WIDTH else None


def clearance_map(cells, r):
    """(size_y, size_x) uint8: 1 where the (2 r + 1)^2 window is on the map and all 0"""
    cells = np.asarray(cells, dtype=np.uint8)
    sy, sx = cells.shape
    blocked = np.ones((sy + 2 * r, sx + 2 * r), dtype=bool)  # off the map counts as blocked
    blocked[r:r + sy, r:r + sx] = cells != 0
    rows = np.zeros((sy + 2 * r, sx), dtype=bool)
    for d in range(2 * r + 1):
        rows |= blocked[:, d:d + sx]
    out = np.zeros((sy, sx), dtype=bool)
    for d in range(2 * r + 1):
        out |= rows[d:d + sy, :]
    return (~out).astype(np.uint8)


K2_FOOTPRINT = [[0.25, 0.0], [-0.25, 0.0]]  # fewer than three vertices: the check reads the centre cell alone
