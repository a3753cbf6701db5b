#!/usr/bin/env python3
"""What the footprint clearance map costs and saves in a blocking step (sfw_set_footprint_clearance):
   python tools/clearance_probe.py [workload] [steps] [rounds] [grid, e.g. 64x64]
Per round, interleaved: the step with the map on and off over an unchanged costmap, and over a costmap that CHANGES before
every step (one far cell toggles, as bench.py's `upload` extra does: the snapshot is re-sent and, with the map on, the map is
built again).  Medians of the blocking step in microseconds, per round, so that the spread between rounds is visible next to
the differences.  Under `rocprofv3 --kernel-trace --stats` the same run gives the build's own kernel times
(sfw_clearance_rows_kernel, sfw_clearance_cols_kernel) and K1b's (sfw_footprint_kernel) with and without the map.
With a library that has no clearance switch (an older build in SFW_HIP_LIB) the "on" rows are left out."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench
from social_force_window_planner_amd import planner

name = sys.argv[1] if len(sys.argv) > 1 else "target"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
bench.GRID_OVERRIDE = sys.argv[4] if len(sys.argv) > 4 else None
job = bench.GridJob(name, "f64", 0, 1, 0)
s, sc = job.scorer, job.scene
has_switch = hasattr(planner.lib(), "sfw_set_footprint_clearance")
cells = sc.cells
c0 = int(cells[1, 1])


def run(on, changing):
    if has_switch:
        s.set_footprint_clearance(on)
    t = []
    for k in range(steps + 3):
        if changing:
            cells[1, 1] = (c0 + 1 + (k & 1)) % 250
        t0 = time.perf_counter()
        if changing:
            s.load_scene(sc)
        job.step()
        t.append(time.perf_counter() - t0)
    cells[1, 1] = c0
    s.load_scene(sc)
    return float(np.median(t[3:]) * 1e6)


for _ in range(5):
    job.step()
if has_switch:
    s.stage(sc.robot_state, job.lin, job.ang, sc.goal_args, job.index_base)
    print(name, "grid %d" % job.n_local, "map %dx%d" % (cells.shape[1], cells.shape[0]), "clearance (built, half_width):", s.footprint_clearance_info())
modes = [(on, ch) for ch in (False, True) for on in ((True, False) if has_switch else (False,))]
for r in range(rounds):
    print(name, f"grid {job.n_local} round {r}:", "  ".join(f"{'on ' if on else 'off'} {'changing' if ch else 'static  '} {run(on, ch):8.1f} us" for on, ch in modes))
