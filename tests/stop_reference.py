"""The stop check's braking tail (sfw_set_stop_check, include/sfw_hip.h) stated through the two references the robot's side
already has.  A plain module: no fixtures, nothing pytest collects, no project code imported.

EXACT LAYER.  The tail IS a rollout: rollout_reference.rollout with every target 0, the braking limits as the acceleration
limits, from the state the rollout left (th_S and the velocities of step S - 1), cut behind the first step whose velocities vx
and vy are both 0 — that step is still integrated and checked — or at max_steps (then UNFINISHED when it still moves).
Velocities, headings and the tail's length are asserted bit for bit (the sign of a zero velocity excepted, as in
rollout_reference); with heading 0 throughout and no lateral velocity the poses are exact-layer too (straight_tail_poses).

HIGH-PRECISION LAYER.  rollout_reference.hp_rollout and pose_bound over the rollout and its tail as ONE sequence of S + m steps
from the handed-over state (hp_poses): the tail's poses inherit the rollout's error, and a step that does not move (a shorter
tail padded to m steps) contributes nothing to either.

VERDICT.  costmap_reference.pose_code over given tail poses in check order: a sample is rejected iff a pose is illegal (a code
below 0, or 254 / 255), hit is the first such pose; UNFINISHED rejects whatever the poses say; a sample is left out (None) when
a pose that matters — any pose up to and including the first illegal one — is in doubt (costmap_reference.in_doubt)."""
import math
from types import SimpleNamespace as NS

import numpy as np

import costmap_reference as CR
import rollout_reference as RR

MAX_STEPS = 4096  # SFW_STOP_MAX_STEPS
NONE, UNFINISHED, NOT_RUN = -1, -2, -3


def end_state(ex, S, poses_S=None):
    """(n, 6) states behind the last step of the exact-layer rollout `ex`: (x_S, y_S) from poses_S (n, 2) (zeros without),
    th_S and the velocities of step S - 1"""
    n = ex.vx.shape[1]
    end = np.zeros((n, 6))
    if poses_S is not None:
        end[:, 0:2] = poses_S
    end[:, 2], end[:, 3], end[:, 4], end[:, 5] = ex.th[S], ex.vx[S - 1], ex.vy[S - 1], ex.vth[S - 1]
    return end


def exact_tail(end, dec, dt, max_steps):
    """end: (n, 6) states (x, y, theta, vx, vy, vtheta).  -> steps (n,), unfinished (n,), vx / vy / vth (m, n): velocities after
    tail step j, th (m + 1, n): heading BEFORE tail step j — th[j + 1] is the heading pose j is checked at; m = max(steps).
    Rows at j >= steps[i] are the rollout run on (what a longer neighbour needs them for: nothing)."""
    assert 1 <= max_steps <= MAX_STEPS
    end = np.ascontiguousarray(end, dtype=np.float64).reshape(-1, 6)
    n = len(end)
    rs = tuple(end[:, c] if n > 1 else float(end[0, c]) for c in range(6))  # (per-sample states: rollout broadcasts them)
    moving0 = (end[:, 3] != 0.0) | (end[:, 4] != 0.0)
    m = min(64, max_steps)
    while True:
        ex = RR.rollout(m, dt, rs, dec, np.zeros((n, 3)))
        moving = (ex.vx != 0.0) | (ex.vy != 0.0)  # after step j
        done = ~moving.all(axis=0) | ~moving0
        if done.all() or m == max_steps:
            break
        m = min(4 * m, max_steps)
    first_rest = np.where(moving.all(axis=0), m, (~moving).argmax(axis=0))
    steps = np.where(moving0, np.minimum(first_rest + 1, m), 0)
    unfinished = moving0 & moving.all(axis=0)  # (only possible at m == max_steps)
    top = int(steps.max()) if n else 0
    return NS(steps=steps, unfinished=unfinished, vx=ex.vx[:top], vy=ex.vy[:top], vth=ex.vth[:top], th=ex.th[:top + 1])


def straight_tail_poses(end, tl, dt):
    """(m, n, 3) tail poses (x, y, th) of tails at heading 0 with no lateral velocity: exact layer (cos = 1, sin = 0)"""
    m, n = tl.vx.shape
    assert np.all(tl.th == 0.0) and np.all(tl.vy == 0.0)
    p = np.zeros((m, n, 3))
    x, y = np.array(end[:, 0], dtype=np.float64), np.array(end[:, 1], dtype=np.float64)
    for j in range(m):
        x = x + (tl.vx[j] * 1.0 + tl.vy[j] * 0.0) * np.float64(dt)
        y = y + (tl.vx[j] * 0.0 + tl.vy[j] * 0.0) * np.float64(dt)
        p[j, :, 0], p[j, :, 1], p[j, :, 2] = x, y, tl.th[j + 1]
    return p


def joined(ex, S, tl):
    """the rollout and its tail as one exact-layer sequence of S + m steps; a tail step at j >= steps[i] does not move"""
    m = tl.vx.shape[0]
    live = np.arange(m)[:, None] < tl.steps[None, :]
    return NS(vx=np.concatenate([ex.vx[:S], np.where(live, tl.vx, 0.0)]), vy=np.concatenate([ex.vy[:S], np.where(live, tl.vy, 0.0)]),
              vth=np.concatenate([ex.vth[:S], tl.vth]), th=np.concatenate([ex.th[:S], tl.th]))


def hp_poses(S, dt, rs, ex, tl, sincos_ulp):
    """-> hp (rollout_reference.hp_rollout over the S + m joined steps), bx, by: (S + m + 1, n) pose bounds.  Tail pose j is
    row S + j + 1."""
    full = joined(ex, S, tl)
    hp = RR.hp_rollout(S + tl.vx.shape[0], dt, rs, (0.0, 0.0), full)
    bx, by = RR.pose_bound(hp, sincos_ulp)
    return hp, bx, by


def verdict(m, footprint, poses, steps, unfinished, tally=None):
    """poses: (n, cap, 3) tail poses in check order, cap >= the steps looked at.  -> per sample (rejected, hit) or None (left
    out).  tally (a dict) counts the poses looked at and the poses in doubt."""
    out = []
    for i in range(len(steps)):
        if unfinished[i]:
            out.append((True, UNFINISHED))
            continue
        hit, doubt = NONE, False
        for j in range(int(steps[i])):
            x, y, th = poses[i, j]
            d = CR.in_doubt(m, footprint, x, y, th)
            if tally is not None:
                tally["poses"] = tally.get("poses", 0) + 1
                tally["left_out"] = tally.get("left_out", 0) + (1 if d else 0)
            if d:
                doubt = True
                break
            code = CR.pose_code(m, footprint, x, y, th)
            if code < 0 or code >= 254:
                hit = j
                break
        out.append(None if doubt else (hit != NONE, hit))
    return out


# ---- the "wall ahead" family: heading 0, no lateral velocity, every pose exact-layer -------------------------------------------------
WALL_DT = 0.25
WALL_GEOMETRY = (37, 23, 0.0, -0.575, 0.05)  # size_x, size_y, origin_x, origin_y, resolution: the robot drives along y = 0
WALL_FOOTPRINT = [[0.1, 0.05], [-0.1, 0.05], [-0.1, -0.05], [0.1, -0.05]]
WALL_X0 = 0.4


def wall_map(wall_cell):
    """a free 37 x 23 map at 0.05 m with one lethal column at cell x = wall_cell (None: no wall, the map's own edge instead)"""
    sx, sy, ox, oy, res = WALL_GEOMETRY
    cells = np.zeros((sy, sx), dtype=np.uint8)
    if wall_cell is not None:
        cells[:, wall_cell] = 254
    return CR.make_map(cells, ox, oy, res)


def wall_case(name, S, lin, acc, dec, max_steps, wall_cell, v0=0.0, ang=(0.0,), acc_theta=None):
    """One launch: the robot at (WALL_X0, 0, 0) moving at v0, the grid lin x ang under acceleration limit acc, S steps of
    WALL_DT, then the tail under (dec, dec, dec).  ang other than 0 only with acc_theta = 0: the heading stays 0, and the
    sample (0, ang) is one a grid scores."""
    acc3 = (float(acc), float(acc), float(acc if acc_theta is None else acc_theta))
    assert all(a == 0.0 for a in ang) or acc3[2] == 0.0
    return NS(name=name, S=S, dt=WALL_DT, lin=np.asarray(lin, dtype=np.float64), ang=np.asarray(ang, dtype=np.float64), acc=acc3,
              dec=(float(dec),) * 3, max_steps=int(max_steps), map=wall_map(wall_cell),
              footprint=np.asarray(WALL_FOOTPRINT, dtype=np.float64), rs=(WALL_X0, 0.0, 0.0, float(v0), 0.0, 0.0),
              goal=acc3 + (1.5, 0.0))


def wall_cases():
    """tails of 0, 1, 3 and about 20 steps; S = 2 and 6; 5 to 12 linvels; from rest and already moving; a lethal column a few
    cells beyond the end of the rollout, or the map's own edge (1.85 m) in its place; one family that ends UNFINISHED"""
    lin5 = [0.1, 0.2, 0.3, 0.4, 0.5]
    lin12 = [0.05 * k for k in range(1, 13)]
    lin_rev = [-0.1, 0.1, 0.2, 0.3, 0.4, 0.5]  # (a reversing sample: the reference's loop would never check it)
    out = []
    for S in (2, 6):
        def wall_of(lin, v0=0.0):  # a cell or two beyond where the fastest sample's front ends a rollout of S + 1 steps
            return min(int((WALL_X0 + max(max(lin), v0) * WALL_DT * (S + 1) + 0.1) / 0.05) + 2, 35)
        # a limit every velocity is inside: the tail is ONE step (to 0) — and 0 steps for the sample that ends at rest, which a
        # grid scores because its angular target is not 0 (the heading stays 0 all the same: no angular acceleration)
        out.append(wall_case(f"S{S}_tail1", S, [0.0] + lin5, 1e3, 1e3, 8, wall_of(lin5), v0=0.0, ang=(0.25,), acc_theta=0.0))
        # 0.1 per step: tails of 1 .. 5 steps (3 among them)
        out.append(wall_case(f"S{S}_tail3", S, lin5, 1e3, 0.4, 64, wall_of(lin5)))
        # 0.025 per step: up to 24 steps, the wall a few cells on
        out.append(wall_case(f"S{S}_tail20", S, lin12, 1e3, 0.1, 64, wall_of(lin12, 0.3), v0=0.3))
        out.append(wall_case(f"S{S}_tail20_edge", S, lin12, 1e3, 0.1, 64, None, v0=0.3))
        out.append(wall_case(f"S{S}_reverse", S, lin_rev, 1e3, 0.4, 64, wall_of(lin_rev, 0.2), v0=0.2))
        # max_steps 4 cuts the longer tails: UNFINISHED beside finished ones
        out.append(wall_case(f"S{S}_unfinished", S, lin5, 1e3, 0.4, 4, None))
    # the rollout itself under a real acceleration limit, the robot already moving
    out.append(wall_case("S6_ramp", 6, lin12, 0.5, 0.15, 128, 30, v0=0.25))
    return out


_WALL = {}


def wall_reference(case, sequence=False):
    """Both halves of a wall case by the references alone, computed once and shared (never written to): ex (the rollout), end
    (n, 6), tail, poses (m, n, 3), rejected_costmap (n,): rejected before the tail, want: per sample (rejected, hit) — NOT_RUN
    where the tail does not run; steps: the expected sfw_stop_rec.steps (0 where it does not run).
    sequence: the launch as two knots over S + 1 steps, the second knot — the samples in reverse order — from step 1 on; a
    list, so no sample is skipped."""
    key = (case.name, sequence)
    if key not in _WALL:
        cmds = RR.product(case.lin, case.ang)
        n = len(cmds)
        S = case.S + 1 if sequence else case.S
        if sequence:
            ex = RR.rollout(S, case.dt, case.rs, case.acc, np.stack([cmds, cmds[::-1]]), (0, 1))
            skipped = np.zeros(n, dtype=bool)
        else:
            ex = RR.rollout(S, case.dt, case.rs, case.acc, cmds)
            skipped = (cmds[:, 0] == 0.0) & (cmds[:, 2] == 0.0)
        p = RR.straight_line_poses(S, case.dt, case.rs, ex)  # (S + 1, n, 2)
        pre = np.zeros(n, dtype=bool)
        for i in range(n):
            for s in range(S):
                code = CR.pose_code(case.map, case.footprint, p[s, i, 0], p[s, i, 1], 0.0)
                if code < 0 or code >= 254:
                    pre[i] = True
                    break
        end = end_state(ex, S, p[S])
        tl = exact_tail(end, case.dec, case.dt, case.max_steps)
        poses = straight_tail_poses(end, tl, case.dt)
        v = verdict(case.map, case.footprint, np.transpose(poses, (1, 0, 2)), tl.steps, tl.unfinished)
        assert all(w is not None for w in v)  # heading 0: nothing is ever in doubt
        not_run = pre | skipped
        want = [(bool(pre[i]), NOT_RUN) if not_run[i] else v[i] for i in range(n)]
        _WALL[key] = NS(S=S, ex=ex, rollout_poses=p, end=end, tail=tl, poses=poses, rejected_costmap=pre, skipped=skipped, want=want,
                              steps=np.where(not_run, 0, tl.steps), cmds=cmds)
    return _WALL[key]


# ---- random headings: what tests/test_stop_check_gpu.py launches, and tests/test_stop_reference.py checks the cap of, on the CPU ------
def random_case(gname, fname, seed, holonomic):
    """96 commands from a rotating robot on a random map: a list with lateral targets (holonomic) or without"""
    geo = CR.geometry(gname)
    rng = np.random.default_rng(seed)
    x0, y0 = CR.mid_cell(geo.origin_x, geo.resolution, geo.size_x), CR.mid_cell(geo.origin_y, geo.resolution, geo.size_y)
    m = CR.random_map(geo, seed, (x0, y0), clear_radius=0.6)
    # ... with a lethal ring 0.8 m around the start: beyond every rollout (0.2 m at most), inside the longer braking paths
    my, mx = np.mgrid[0:geo.size_y, 0:geo.size_x]
    d = np.hypot(geo.origin_x + (mx + 0.5) * geo.resolution - x0, geo.origin_y + (my + 0.5) * geo.resolution - y0)
    cells = m.cells.copy()
    cells[(d > 0.8) & (d < 0.9)] = 254
    m = CR.make_map(cells, geo.origin_x, geo.origin_y, geo.resolution)
    n = 96
    cmds = np.stack([rng.uniform(0.1, 0.6, n), rng.uniform(-0.3, 0.3, n) if holonomic else np.zeros(n), rng.uniform(-0.5, 0.5, n)], axis=1)
    rs = (x0, y0, float(rng.uniform(-math.pi, math.pi)), 0.4, 0.05 if holonomic else 0.0, 0.4)  # a rotating robot
    return NS(name=f"{gname}_{fname}_{seed}_{'vy' if holonomic else 'grid'}", map=m, footprint=CR.FOOTPRINTS[fname], rs=rs, cmds=cmds,
                 acc=(1.0, 0.7, 1.3), dec=(0.4, 0.3, 1.0), S=3, dt=0.125, max_steps=64)


RANDOM_CASES = [("wide_120x80_r0.05", "polygon16", 7, False), ("tall_80x120_r0.07", "box", 8, True)]


def random_reference(case):
    """both layers of a random case: ex, tail, hp, bx, by (hp_poses over the joined S + m steps)"""
    ex = RR.rollout(case.S, case.dt, case.rs, case.acc, case.cmds)
    tl = exact_tail(end_state(ex, case.S), case.dec, case.dt, case.max_steps)
    hp, bx, by = hp_poses(case.S, case.dt, case.rs, ex, tl, RR.SINCOS_ULP_DEVICE)
    return ex, tl, hp, bx, by
