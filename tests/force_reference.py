"""The force terms of the model in mpmath.  A plain module: no fixtures, nothing pytest collects.

What csrc/sfw_kernels.hip evaluates with hardware seeds, short polynomials and log2-unit constants (pair_force, obstacle_term /
obstacle_scale, desired_force, group_force, agent_step) and oracle/sfw_oracle.cpp with libm in double, stated once more as the
mathematics they both restate (lightsfm), at PREC bits.  The parameters come from an SfwParams, every
input is a double taken exactly.  tests/test_force_reference.py holds this module to the oracle on any machine;
tests/test_force_terms_gpu.py holds the kernels to it through row 0 of a one-step sfw_score_one_crowd.

Every function returns, next to its value, the figures an error bound needs: the exponent parts x_d = d / B and
x_v / x_a = (n' B theta)^2 / (n B theta)^2 of the pair term, the magnitudes of the two exponentials, and sum |term| of every
sum.  Nothing here has a special case for a pair whose w x diff is exactly 0 beyond sign(0) = 0: the callers keep such pairs out
(the reference's value there is the rounding noise of two atan2, tests/test_parity_holes_gpu.py)."""
import functools
import math
from types import SimpleNamespace as NS

import mpmath as mp
import numpy as np

PREC = 160


def _hp(fn):
    @functools.wraps(fn)
    def run(*a, **kw):
        with mp.workprec(PREC):
            return fn(*a, **kw)
    return run


def _m(v):
    return v if isinstance(v, mp.mpf) else mp.mpf(float(v))


def _norm(x, y):
    return mp.sqrt(x * x + y * y)


def state_of(agent):
    """(x, y, vx, vy) of an SfwAgent"""
    return (agent.x, agent.y, agent.vx, agent.vy)


@_hp
def constants(p):
    """The six log2-unit constants of sfw_derive as they should be: -log2(e)/gamma, log2 Fs, -(n' gamma)^2 log2 e,
    -(n gamma)^2 log2 e, log2 k_obs, log2(e)/sigma"""
    l2e = 1 / mp.log(2)
    g, n, npr = _m(p.sfm_gamma), _m(p.sfm_n), _m(p.sfm_n_prime)
    return NS(neg_l2e_inv_gamma=-l2e / g, l2_f_social=mp.log(_m(p.sfm_force_factor_social), 2) if p.sfm_force_factor_social > 0 else -mp.inf,
              c_vel=-(npr * g) ** 2 * l2e, c_ang=-(n * g) ** 2 * l2e, l2_f_obstacle=mp.log(_m(p.sfm_force_factor_obstacle), 2),
              l2e_inv_sigma=l2e / _m(p.sfm_force_sigma_obstacle))


@_hp
def pair(p, me, other):
    """Force on `me` from `other` (one term of computeSocialForce), both (x, y, vx, vy):
        diff = p_other - p_me, dhat = diff / |diff|, w = v_me - v_other, I = lambda w + dhat, B = gamma |I|,
        theta = angle(dhat) - angle(I) in (-pi, pi] = atan2(I x dhat, I . dhat),
        f = Fs (-exp(-d/B - (n' B theta)^2) Ihat - sign(theta) exp(-d/B - (n B theta)^2) leftNormal(Ihat)).
    ev, ea: the two magnitudes Fs exp(..); norm = |f| = sqrt(ev^2 + ea^2) (ev alone when sign(theta) = 0)."""
    mx, my, mvx, mvy = (_m(v) for v in me)
    ox, oy, ovx, ovy = (_m(v) for v in other)
    lam, gam, n, npr, fs = (_m(getattr(p, k)) for k in ("sfm_lambda", "sfm_gamma", "sfm_n", "sfm_n_prime", "sfm_force_factor_social"))
    dx, dy, wx, wy = ox - mx, oy - my, mvx - ovx, mvy - ovy
    cw = wx * dy - wy * dx
    d = _norm(dx, dy)
    ux, uy = (dx / d, dy / d) if d > 0 else (dx, dy)  # Vector2d::normalized() leaves the zero vector
    ix, iy = lam * wx + ux, lam * wy + uy
    il = _norm(ix, iy)
    assert il > 0, "lambda w = -dhat: the model has no value"
    gx, gy = ix / il, iy / il
    theta = mp.atan2(ix * uy - iy * ux, ix * ux + iy * uy)
    b = gam * il
    x_d, x_v, x_a = d / b, (npr * b * theta) ** 2, (n * b * theta) ** 2
    ev, ea = fs * mp.exp(-x_d - x_v), fs * mp.exp(-x_d - x_a)
    s = mp.sign(theta)
    ea_s = ea if s != 0 else mp.mpf(0)
    return NS(fx=-ev * gx + s * ea * gy, fy=-ev * gy - s * ea * gx, norm=_norm(ev, ea_s), theta=theta, cw=cw, d=d, il=il,
              x_d=x_d, x_v=x_v, x_a=x_a, ev=ev, ea=ea_s)


@_hp
def obstacle(p, pos, radius, points):
    """computeObstacleForce: the mean over the points of k exp(-(|p - o| - radius)/sigma) (p - o)/|p - o| (a coincident point
    adds 0).  terms: (|term| / O, |p - o| / sigma) per point; sum_abs their sum."""
    k, sig, rad = _m(p.sfm_force_factor_obstacle), _m(p.sfm_force_sigma_obstacle), _m(radius)
    px, py = _m(pos[0]), _m(pos[1])
    n = len(points)
    fx = fy = sum_abs = mp.mpf(0)
    terms = []
    for o in points:
        mx, my = px - _m(o[0]), py - _m(o[1])
        m = _norm(mx, my)
        if m == 0:
            terms.append((mp.mpf(0), mp.mpf(0)))
            continue
        mag = k * mp.exp(-(m - rad) / sig) / n
        fx += mag * mx / m
        fy += mag * my / m
        sum_abs += mag
        terms.append((mag, m / sig))
    return NS(fx=fx, fy=fy, norm=_norm(fx, fy), sum_abs=sum_abs, terms=terms, x_r=abs(rad) / sig)


@_hp
def desired(p, state, goal, desired_velocity):
    """computeDesiredForce: k_d (dir v_des - v) / tau towards a goal (gx, gy, radius) farther than its radius, -v / tau without
    one (goal None) or inside it.  dir: the unit direction or (0, 0); en: the distance to the goal (None without one)."""
    x, y, vx, vy = (_m(v) for v in state)
    kd, tau, dv = _m(p.sfm_force_factor_desired), _m(p.sfm_relaxation_time), _m(desired_velocity)
    if goal is not None:
        ex, ey = _m(goal[0]) - x, _m(goal[1]) - y
        en = _norm(ex, ey)
        if en > _m(goal[2]):
            dx, dy = ex / en, ey / en
            return NS(fx=kd * (dx * dv - vx) / tau, fy=kd * (dy * dv - vy) / tau, dir=(dx, dy), en=en,
                      abs_x=kd * (abs(dx) * dv + abs(vx)) / tau, abs_y=kd * (abs(dy) * dv + abs(vy)) / tau)
    else:
        en = None
    return NS(fx=-vx / tau, fy=-vy / tau, dir=(mp.mpf(0), mp.mpf(0)), en=en, abs_x=abs(vx) / tau, abs_y=abs(vy) / tau)


@_hp
def group(p, agents, index, direction):
    """computeGroupForce (non-_PAPER_VERSION_ branch, as oracle/sfw_oracle.cpp sfm_group states it) on agents[index]; `direction`
    its desired direction (desired().dir).  agents: objects with x, y, radius, group_id.
        gaze: the centre of mass of the OTHER members more than 90 degrees off the direction (dir . rel < 0):
              k_g (dir . rel / |dir|^2) dir;
        coherence: (centre - p) k_c (tanh(|centre - p| - (n - 1)/2) + 1) / 2;
        repulsion: k_r sum of (p - p_m) over the members closer than the two radii.
    x_c = |centre - p| - (n - 1)/2, soft = (tanh(x_c) + 1)/2, ep = dir . rel and ep_abs = |dir_x rel_x| + |dir_y rel_y|."""
    a = agents[index]
    zero = mp.mpf(0)
    members = [m for m in range(len(agents)) if a.group_id >= 0 and agents[m].group_id == a.group_id]
    if len(members) < 2:
        return NS(fx=zero, fy=zero, n=len(members), gaze=(zero, zero), coh=(zero, zero), rep=(zero, zero))
    n = mp.mpf(len(members))
    px, py = _m(a.x), _m(a.y)
    cx, cy = sum(_m(agents[m].x) for m in members) / n, sum(_m(agents[m].y) for m in members) / n
    ddx, ddy = direction
    rx, ry = (n * cx - px) / (n - 1) - px, (n * cy - py) / (n - 1) - py
    ep = ddx * rx + ddy * ry
    kg, kc, kr = (_m(getattr(p, "sfm_force_factor_group_" + k)) for k in ("gaze", "coherence", "repulsion"))
    gaze = (kg * ep * ddx, kg * ep * ddy) if ep < 0 else (zero, zero)  # |dir| = 1 wherever ep != 0
    qx, qy = cx - px, cy - py
    dist = _norm(qx, qy)
    x_c = dist - (n - 1) / 2
    soft = (mp.tanh(x_c) + 1) / 2
    coh = (qx * kc * soft, qy * kc * soft)
    sx = sy = sax = say = zero
    for m in members:
        if m == index:
            continue
        ex, ey = px - _m(agents[m].x), py - _m(agents[m].y)
        if _norm(ex, ey) < _m(a.radius) + _m(agents[m].radius):
            sx, sy, sax, say = sx + ex, sy + ey, sax + abs(ex), say + abs(ey)
    rep = (kr * sx, kr * sy)
    return NS(fx=gaze[0] + coh[0] + rep[0], fy=gaze[1] + coh[1] + rep[1], n=len(members), gaze=gaze, coh=coh, rep=rep, centre=(cx, cy),
              rel=(rx, ry), ep=ep, ep_abs=abs(ddx * rx) + abs(ddy * ry), dist=dist, x_c=x_c, soft=soft, rep_abs=(kr * sax, kr * say))


def _goal_of(a):
    return (a.goal_x, a.goal_y, a.goal_radius) if a.has_goal else None


@_hp
def forces(p, agents, points, pairs=None):
    """Every agent's force at the handed-over state, term by term: per agent an NS(desired, obstacle, group, pairs = {j: pair},
    social = (fx, fy, sum of the |f_j|), fx, fy = the global force).  The pair term is antisymmetric in the model (every agent
    carries the same parameters), so an unordered pair is evaluated once.  pairs: a dict to share the evaluations through."""
    A = len(agents)
    pairs = {} if pairs is None else pairs
    out = []
    for i in range(A):
        for j in range(i + 1, A):
            if (i, j) not in pairs:
                f = pair(p, state_of(agents[i]), state_of(agents[j]))
                pairs[(i, j)] = f
                pairs[(j, i)] = NS(**{**vars(f), "fx": -f.fx, "fy": -f.fy, "cw": f.cw})
    grouped = any(a.group_id >= 0 for a in agents)
    for i in range(A):
        a = agents[i]
        des = desired(p, state_of(a), _goal_of(a), a.desired_velocity)
        obs = obstacle(p, (a.x, a.y), a.radius, points) if len(points) else NS(fx=mp.mpf(0), fy=mp.mpf(0), norm=mp.mpf(0), sum_abs=mp.mpf(0), terms=[], x_r=mp.mpf(0))
        grp = group(p, agents, i, des.dir) if grouped else NS(fx=mp.mpf(0), fy=mp.mpf(0), n=0)
        mine = {j: pairs[(i, j)] for j in range(A) if j != i}
        sx, sy = sum((f.fx for f in mine.values()), mp.mpf(0)), sum((f.fy for f in mine.values()), mp.mpf(0))
        out.append(NS(desired=des, obstacle=obs, group=grp, pairs=mine, social=(sx, sy, sum((f.norm for f in mine.values()), mp.mpf(0))),
                      fx=des.fx + sx + obs.fx + grp.fx, fy=des.fy + sy + obs.fy + grp.fy))
    return out


@_hp
def one_step(p, agents, points, dt, robot_after, pairs=None):
    """Row 0 of a rollout: sfm.computeForces at the handed-over state, updatePosition of every person (agent 0, the robot, is
    overwritten with robot_after = (x, y, vx, vy)), computeSocialWork.  Returns NS(forces, state = [(x, y, vx, vy)] of the people
    (index a - 1), clamped = [bool], wr = |social force on the robot| + |its obstacle force|, wp = [pair(person a after the step,
    robot after the step)], social = wr + sum |wp|)."""
    fr = forces(p, agents, points, pairs)
    h = _m(dt)
    state, clamped, wp = [], [], []
    for a in range(1, len(agents)):
        ag = agents[a]
        vx, vy = _m(ag.vx) + fr[a].fx * h, _m(ag.vy) + fr[a].fy * h
        sp, dv = _norm(vx, vy), _m(ag.desired_velocity)
        clamped.append(sp > dv)
        if sp > dv:
            vx, vy = vx / sp * dv, vy / sp * dv
        state.append((_m(ag.x) + vx * h, _m(ag.y) + vy * h, vx, vy))
        wp.append(pair(p, state[-1], robot_after))
    wr = _norm(fr[0].social[0], fr[0].social[1]) + fr[0].obstacle.norm
    return NS(forces=fr, state=state, clamped=clamped, wr=wr, wp=wp, social=wr + sum((w.norm for w in wp), mp.mpf(0)))


# ---- constructed inputs ---------------------------------------------------------------------------------------------------------
# Every coordinate and velocity lies on the grid 2^-20 with |value| < 2^11: differences of two of them and w x diff are exact in
# double, so the sign of theta the kernels read off w x diff is the mathematical one.
GRID = 2.0 ** -20


def on_grid(v):
    return round(float(v) * 2 ** 20) / 2 ** 20


def pair_from_polar(p, d, alpha, il, theta):
    """(dx, dy, wx, wy) on the grid whose pair term has |diff| = d in direction alpha, |I| = il and angle theta — up to the
    rounding to the grid: w = (I - dhat) / lambda with I = il (cos, sin)(alpha - theta)"""
    dx, dy = d * math.cos(alpha), d * math.sin(alpha)
    ix, iy = il * math.cos(alpha - theta), il * math.sin(alpha - theta)
    return (on_grid(dx), on_grid(dy), on_grid((ix - dx / d) / p.sfm_lambda), on_grid((iy - dy / d) / p.sfm_lambda))


FOLD_ANGLES = ("pi/4", "pi/2", "3pi/4")


def pair_cases(p, n, seed, d_range=(0.3, 6.0), il_range=(0.2, 4.0)):
    """n pair inputs (dx, dy, wx, wy) by construction from (|diff|, direction, |I|, theta): |theta| at 2^-10, the three fold
    angles of angle_abs +- 2^-20, pi - 2^-10 and uniform, both signs, directions uniform.  Pairs whose w x diff came out 0 are
    replaced by the next draw (the count stays n)."""
    rng = np.random.default_rng(seed)
    special = [2.0 ** -10, math.pi / 4 - 2.0 ** -20, math.pi / 4 + 2.0 ** -20, math.pi / 2 - 2.0 ** -20, math.pi / 2 + 2.0 ** -20,
               3 * math.pi / 4 - 2.0 ** -20, 3 * math.pi / 4 + 2.0 ** -20, math.pi - 2.0 ** -10]
    out = []
    while len(out) < n:
        k = len(out) % (2 * len(special))
        th = special[k // 2] if k % 2 == 0 else rng.uniform(0.0, math.pi)
        th *= rng.choice([-1.0, 1.0])
        c = pair_from_polar(p, rng.uniform(*d_range), rng.uniform(-math.pi, math.pi), rng.uniform(*il_range), th)
        if c[2] * c[1] - c[3] * c[0] != 0.0:
            out.append(c)
    return out


def exact_fold_cases(p):
    """theta exactly +-pi/4, +-pi/2, +-3pi/4 (I = s (1, -+1), s (0, -+1), s (-1, -+1) against dhat = (1, 0), and the same turned by
    90 degrees): needs 1 / lambda on the grid"""
    out = []
    for d in (0.5, 2.0):
        for s in (0.25, 1.0):
            for ix, iy in ((s, s), (s, -s), (0.0, s), (0.0, -s), (-s, s), (-s, -s)):
                wx, wy = (ix - 1.0) / p.sfm_lambda, iy / p.sfm_lambda
                assert on_grid(wx) == wx and on_grid(wy) == wy
                out.append((d, 0.0, wx, wy))
                out.append((0.0, d, -wy, wx))
    return out


# the default and two more parameter sets: between them every constant sfw_derive forms differs from the default's, n and n'
# are once far apart and once nearly equal, and Fs is once below 1 (log2 Fs < 0) and once large
PARAM_SETS = {
    "default": {},
    "wide": dict(sfm_lambda=0.5, sfm_gamma=0.1, sfm_n=1.0, sfm_n_prime=0.5, sfm_force_factor_social=2.0 ** -8, sfm_force_sigma_obstacle=0.5,
                 sfm_force_factor_obstacle=3.0, sfm_relaxation_time=0.25, sfm_force_factor_desired=3.0, sfm_force_factor_group_gaze=1.5,
                 sfm_force_factor_group_coherence=0.75, sfm_force_factor_group_repulsion=2.5),
    "near": dict(sfm_lambda=1.0, sfm_gamma=0.5, sfm_n=2.0, sfm_n_prime=2.0625, sfm_force_factor_social=1000.0, sfm_force_sigma_obstacle=0.125,
                 sfm_force_factor_obstacle=0.75, sfm_relaxation_time=2.0, sfm_force_factor_desired=0.5),
}
FAST = 64.0  # a desired velocity no one-step scene reaches: the speed clamp of updatePosition stays out of the way


def agent(x, y, vx=0.0, vy=0.0, goal=None, goal_radius=0.25, desired_velocity=FAST, radius=0.375, ident=0, group_id=-1):
    """an SfwAgent on the grid (asserted)"""
    from social_force_window_planner_amd._abi import SfwAgent
    a = SfwAgent()
    a.x, a.y, a.vx, a.vy = float(x), float(y), float(vx), float(vy)
    if goal is not None:
        a.goal_x, a.goal_y, a.has_goal = float(goal[0]), float(goal[1]), 1
    a.goal_radius, a.desired_velocity, a.radius, a.id, a.group_id = goal_radius, desired_velocity, radius, ident, group_id
    for v in (a.x, a.y, a.vx, a.vy, a.goal_x, a.goal_y):
        assert on_grid(v) == v and abs(v) < 2 ** 11, v
    return a


def agent_array(agents):
    from social_force_window_planner_amd._abi import SfwAgent
    arr = (SfwAgent * len(agents))(*agents)
    for i in range(len(agents)):
        arr[i].id = i
    return arr


def all_pairs_turn(agents):
    """w x diff != 0 for every pair (exact: the inputs are on the grid)"""
    for i in range(len(agents)):
        for j in range(i + 1, len(agents)):
            a, b = agents[i], agents[j]
            if (a.vx - b.vx) * (b.y - a.y) - (a.vy - b.vy) * (b.x - a.x) == 0.0:
                return False
    return True


def _grid_draw(rng, lo, hi, size=None, bits=10):
    return np.round(rng.uniform(lo, hi, size) * 2 ** bits) / 2 ** bits


def ring_points(n, radius, centre=(0.0, 0.0), phase=0.0):
    if n == 0:
        return np.zeros((0, 2))
    a = phase + np.arange(n) * (2.0 * math.pi / n)
    return np.stack([[on_grid(v) for v in centre[0] + radius * np.cos(a)], [on_grid(v) for v in centre[1] + radius * np.sin(a)]], axis=1)


def mixed_scene(n_agents, n_points, seed, desired_velocity=FAST):
    """The robot at the origin, n_agents - 1 walking people at least 1 m from it and 0.75 m apart, each with a goal, people 2..4
    a group (when there are that many), n_points laser points on a ring of 3.5 m turned off the axes.  Returns (agents, points)."""
    rng = np.random.default_rng(seed)
    people, r_out = [], max(4.0, math.sqrt(n_agents))
    while len(people) < n_agents - 1:
        x, y = _grid_draw(rng, -r_out, r_out, 2)
        if x * x + y * y >= 1.5 ** 2 and all((x - q[0]) ** 2 + (y - q[1]) ** 2 >= 0.75 ** 2 for q in people):
            people.append((x, y))
    agents = [agent(0.0, 0.0, 0.40625, 0.03125, desired_velocity=0.75)]
    for i, (x, y) in enumerate(people):
        vx, vy = _grid_draw(rng, -1.25, 1.25, 2, bits=20)
        gx, gy = _grid_draw(rng, -3.0, 3.0, 2)
        agents.append(agent(x, y, vx, vy, goal=(x + gx, y + gy), desired_velocity=desired_velocity,
                            group_id=7 if 1 <= i <= 3 and n_agents >= 5 else -1))
    agents = agent_array(agents)
    assert all_pairs_turn(agents)
    return agents, ring_points(n_points, 3.5, phase=0.1)


def group_scenes(desired_velocity=2.0):
    """{name: agents}: the robot far away, every person a member of one group, distinct velocities below 1 m/s per component,
    goals in different directions (gaze on both sides of dir . rel = 0, one member without a goal).  The desired velocity is low,
    so that the desired force does not drown the group force in a sum: a caller picks the step short enough for the clamp.
      two<s>: two members s apart: coherence at |centre - p| - (n - 1)/2 = (s - 1)/2 = 0, 1, 40, 400;
      three: one member at the centre of the other two (-1);   eight: scattered;   many: 82 members, two of them 0.5 from the
      centre (-40);   touch: members just inside, at and just outside the sum of their radii (repulsion on both sides)."""
    rng = np.random.default_rng(5)
    robot = agent(-20.0, -24.0, 0.40625, 0.03125, desired_velocity=0.75)

    def members(positions, radius=0.375, goal_free=None):
        out = [robot]
        for i, (x, y) in enumerate(positions):
            vx, vy = _grid_draw(rng, -1.0, 1.0, 2, bits=20)
            gx, gy = _grid_draw(rng, 1.0, 3.0) * rng.choice([-1.0, 1.0]), _grid_draw(rng, 1.0, 3.0) * rng.choice([-1.0, 1.0])
            out.append(agent(x, y, vx, vy, goal=None if i == goal_free else (x + gx, y + gy), radius=radius, group_id=3,
                             desired_velocity=desired_velocity))
        arr = agent_array(out)
        assert all_pairs_turn(arr)
        return arr

    scenes = {f"two{s}": members([(1.0 - s / 2.0, 0.5), (1.0 + s / 2.0, 0.5)]) for s in (1, 3, 81, 801)}
    scenes["three"] = members([(0.25, -0.5), (1.75, 0.5), (-1.25, -1.5)], goal_free=2)
    scenes["eight"] = members([tuple(_grid_draw(rng, -3.0, 3.0, 2)) for _ in range(8)], radius=0.25, goal_free=5)
    lattice = [(0.5, 0.0)] + [(2.0 * i, 2.0 * j + 1.0) for i in range(-4, 5) for j in range(0, 5)][:40]
    scenes["many"] = members(lattice + [(-x, -y) for x, y in lattice], radius=0.125)
    scenes["touch"] = members([(0.0, 0.0), (0.75 - GRID, 0.0), (0.0, 0.75), (-0.75 - GRID, 0.0), (0.5, -0.5)], goal_free=4)
    return scenes
