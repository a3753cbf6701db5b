"""The force terms of the kernels against mpmath, one term at a time, through the public ABI.

Every other comparison of a force with a reference goes through the CPU oracle at 1e-9 (1e-4 for SFW_PRECISION_F32); the kernels
are good to a few 1e-14, so a constant of sfw_derive rounded through float, n used for n', a dropped sign transfer or a missing
factor in an exponent passes all of them.  Here row 0 of a ONE-step rollout (sim_time = sim_granularity = dt, a power of two) is
one force evaluation at the handed-over state (sfw_score_one_crowd):
  * person a:  state[0][a].v = v + F dt, F = desired + sum of pair terms + laser-point mean + group force — one fma, one rounding;
  * work[0][0] = |sum_j pair(robot <- j)| + |laser-point force on the robot| at the handed-over state;
  * work[0][a] = |pair(person a <- robot)| at the returned row: the reference takes the returned doubles as its inputs.
The scoring kernels (one-launch cycle, register form, flat form, sample list) are held to the same references through
SFW_TERM_SOCIAL of sfw_grid_terms.  The robot moves without acceleration (acc = 0: every sample of a grid makes the same step),
by a displacement that keeps it clear of the contact radius; desired velocities are out of reach (no speed clamp) and asserted so.

Inputs lie on the grid 2^-20 (tests/force_reference.py): w x diff is exact, and every scene asserts it non-zero for every pair —
exact relative rest and collinear motion are lightsfm's rounding-noise cases (tests/test_parity_holes_gpu.py), not cases here.

BOUNDS.  Derived, not tuned: first-order propagation of the bounds of profiles/r18_device_math.txt (the `bound` column — what
tests/test_device_math_gpu.py asserts of the building blocks — of the rows of the precision mode: exp2, angle_abs composed
(absolute, radians), refined rsqrt / sqrt, reciprocal) plus u = 2^-53 (2^-24 where the force type is float) per IEEE operation:
    one exponential with exponent parts x_d, x_t:
        E = E_exp + x_d (2 E_rs + 4 u) + 2 u |ln Fs| + x_t (2 E_ang / |theta| + 2 E_rs + 6 u)
    (the two roundings that form log2 Fs - x_d log2 e act on the whole exponent, hence the |ln Fs| share);
    pair force:  |fv| (E_v + E_rs + 4 u) + |fa| (E_a + E_rs + 4 u);   a norm adds (E_rs + 4 u) |f|;
    laser point: |term| (E_exp + x_o (E_rs + 3 u) + E_rs + 3 u), the agent's factor E_exp + 2 u (x_r + |ln k|) + 3 u, the sum
                 (ceil(O / 16) + 16) u of sum |term|;
    desired force: (E_rs + 6 u) k (|dir| v_des + |v|) / tau per component;
    group force: see group_model;   a sum of n terms: n u sum |term|;   a velocity: u |v'| / dt per component.
Asserted: 2 x the model (the margin of tests/test_device_math_gpu.py) + the floors, all absolute and far below anything a sum can
tell: an exponential below 2^-1022 (2^-126 in float) is +0 on the device, two of them per pair; a laser point's exponential and
its quotient by the distance likewise, before the distance vector and the agent's factor multiply them (obstacle_floor); a
double norm below 1e-150 is not resolved (NORM_FLOOR: the robot's work entry IS the scoring pass's addend); a person's work in
a SCORING kernel has the floor of its norm q rsqrt(q + tiny) (sfw_kernels.hip small_wp: 0.3 sqrt(tiny)), which the capture
evaluates again.
`python tests/test_force_terms_gpu.py` prints the worst ratio to the model per term and mode: profiles/r20_force_terms.txt."""
import math
import os
import sys

import mpmath as mp
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (run as a script for the table; under pytest tests/conftest.py has done it)
    sys.path.insert(0, ROOT)

import force_reference as F  # noqa: E402
from social_force_window_planner_amd import synthetic as syn  # noqa: E402
from social_force_window_planner_amd._abi import (SFW_K2_FLAT, SFW_K2_REGISTER, SFW_ORG_FLAT, SFW_ORG_REGISTER_1, SFW_ORG_REGISTER_2,  # noqa: E402
                                                   SFW_PRECISION_F32, SFW_PRECISION_F64, SFW_PRECISION_F64_STRICT, SFW_TERM_SOCIAL,
                                                   default_params)

pytestmark = pytest.mark.gpu

PRECISIONS = [SFW_PRECISION_F64, SFW_PRECISION_F64_STRICT, SFW_PRECISION_F32]
MODE_NAME = {SFW_PRECISION_F64: "f64", SFW_PRECISION_F64_STRICT: "f64 strict", SFW_PRECISION_F32: "f32"}
SOCIAL_ONLY = dict(vel_weight=0.0, distance_weight=0.0, angle_weight=0.0, costmap_weight=0.0, social_weight=1.0)
U64 = 2.0 ** -53
MARGIN = 2.0
ROBOT_RADIUS = float(np.float32(0.35))
NORM_FLOOR = 1e-150  # fast_norm (sfw_kernels.hip) is q rsqrt(max(q, 1e-300)), q = x^2 + y^2: below 1e-150 a double norm is not resolved
GOAL_ARGS = (0.0, 0.0, 0.0, 2.0, 0.5)  # no acceleration: the robot keeps the velocity of its state, whatever the sample


def device_math_bounds():
    """{(function, build): bound} of profiles/r18_device_math.txt"""
    out = {}
    for line in open(os.path.join(ROOT, "profiles", "r18_device_math.txt")):
        cells = [c.strip() for c in line.split("|")]
        if len(cells) >= 4 and cells[1] in ("default", "strict"):
            try:
                out[(cells[0], cells[1])] = float(cells[3])
            except ValueError:
                pass
    return out


class Mode:
    """the figures of one precision mode: of the force type (pair term, laser points) and of the double path (desired and group
    force, norms, the Euler step), which every mode shares but for the strict build's longer asin"""

    def __init__(self, precision):
        b = device_math_bounds()
        build = "strict" if precision == SFW_PRECISION_F64_STRICT else "default"
        self.precision, self.name = precision, MODE_NAME[precision]
        self.d_exp, self.d_rs, self.d_rcp = b[("exp2_fast", build)], max(b[("rsqrt", build)], b[("sqrt", build)]), b[("rcp_nr", build)]
        if precision == SFW_PRECISION_F32:
            self.u, self.e_exp, self.e_ang = 2.0 ** -24, b[("exp2_fast f32", build)], b[("angle_abs f32", build)]
            self.e_rs, self.floor, self.floor_scoring = max(b[("rsqrt f32", build)], b[("sqrt f32", build)]), 2.0 ** -125, 2.0 ** -51
            self.smallest = 2.0 ** -126
        else:
            self.u, self.e_exp, self.e_ang = U64, self.d_exp, b[("angle_abs composed", build)]
            self.e_rs, self.floor, self.floor_scoring = self.d_rs, 2.0 ** -1021, 2.0 ** -500
            self.smallest = 2.0 ** -1022


# ---- the error model --------------------------------------------------------------------------------------------------------------
def pair_model(m, p, r):
    """absolute bound of a pair force vector (and of each component) for a force_reference.pair result"""
    th = abs(float(r.theta))
    ln_fs = abs(math.log(p.sfm_force_factor_social)) if p.sfm_force_factor_social > 0 else 0.0
    ang = 2.0 * m.e_ang / th if th > 0 else 0.0

    def e(x_t):
        return m.e_exp + float(r.x_d) * (2 * m.e_rs + 4 * m.u) + 2 * m.u * ln_fs + float(x_t) * (ang + 2 * m.e_rs + 6 * m.u)
    ihat = m.e_rs + 4 * m.u
    return float(r.ev) * (e(r.x_v) + ihat) + float(r.ea) * (e(r.x_a) + ihat)


def obstacle_model(m, p, o):
    if not o.terms:
        return 0.0
    n = len(o.terms)
    per_term = sum(float(mag) * (m.e_exp + float(x) * (m.e_rs + 3 * m.u) + m.e_rs + 3 * m.u) for mag, x in o.terms)
    factor = m.e_exp + 2 * m.u * (float(o.x_r) + abs(math.log(p.sfm_force_factor_obstacle))) + 3 * m.u
    return per_term + float(o.sum_abs) * (factor + (math.ceil(n / 16) + 16) * m.u)


def obstacle_floor(m, p, o):
    """what the flush costs the laser-point mean: a point's 2^(-|p - o| log2(e)/sigma) and its product with 1 / |p - o| are +0
    below the smallest normal of the force type, before (p - o) and the agent's factor k exp(radius/sigma) / O multiply them"""
    if not o.terms:
        return 0.0
    sigma = p.sfm_force_sigma_obstacle
    factor = p.sfm_force_factor_obstacle * math.exp(float(o.x_r)) / len(o.terms)
    return m.smallest * factor * sum(1.0 + float(x) * sigma for _, x in o.terms)


def desired_model(m, d):
    return (m.d_rs + 6 * U64) * float(max(d.abs_x, d.abs_y))


def group_model(m, p, agent, des, g):
    """group_force, double in every mode.  With c the centre, n members, positions of magnitude P = |c| + |p|:
      centre: c = csum rcp(n): |c| (E_rcp + (n + 1) u) per component;
      gaze: rel = rcp(n - 1) (n c - p) - p inherits 2 (n / (n - 1)) of the centre's error and (E_rcp + 4 u) P; dir (E_rs + 2 u);
            k_g (dir . rel) dir: the products of dir . rel at their magnitudes;
      coherence: soft = rcp(1 + 2^(-2 x_c log2 e)): E_rcp + 3 u + w (E_exp + the error of 2 x_c), w = 1 - soft the share of the
            exponential in the denominator, x_c = dist - (n - 1)/2 with dist from the refined root;
      repulsion: the differences are exact on the grid, the sum and the product one rounding each."""
    if g.n < 2:
        return 0.0
    n = g.n
    kg, kc = p.sfm_force_factor_group_gaze, p.sfm_force_factor_group_coherence
    c_err = [abs(float(g.centre[c])) * (m.d_rcp + (n + 1) * U64) for c in (0, 1)]
    pos = (abs(agent.x), abs(agent.y))
    rel_err = [2.0 * n / (n - 1) * c_err[c] + (m.d_rcp + 4 * U64) * (abs(float(g.centre[c])) * n / (n - 1) + pos[c] * (1 + 1 / (n - 1))) for c in (0, 1)]
    dd = [abs(float(v)) for v in des.dir]
    ep_err = dd[0] * rel_err[0] + dd[1] * rel_err[1] + (m.d_rs + 4 * U64) * float(g.ep_abs)
    gaze = kg * (ep_err + (m.d_rs + 4 * U64) * float(g.ep_abs)) * max(dd)
    dist, soft = float(g.dist), float(g.soft)
    x_err = 2.0 * (dist * (m.d_rs + 3 * U64) + c_err[0] + c_err[1]) + 4 * U64 * abs(2.0 * float(g.x_c))
    soft_rel = m.d_rcp + 4 * U64 + (1.0 - soft) * (m.d_exp + x_err)
    coh = kc * soft * (dist * soft_rel + max(c_err))
    rep = 3 * U64 * float(max(g.rep_abs))
    return gaze + coh + rep


def force_model(m, p, agents, a, f):
    """absolute bound of each component of the whole force on person a (force_reference.forces entry f)"""
    pairs = sum(pair_model(m, p, r) for r in f.pairs.values())
    total = float(f.social[2]) + float(f.obstacle.sum_abs) + float(max(f.desired.abs_x, f.desired.abs_y)) + abs(float(f.group.fx)) + abs(float(f.group.fy))
    grp = group_model(m, p, agents[a], f.desired, f.group) if f.group.n >= 2 else 0.0
    return pairs + obstacle_model(m, p, f.obstacle) + desired_model(m, f.desired) + grp + (len(f.pairs) + 6) * U64 * total


def ratio(err, floor, model):
    """the error beyond the flush floor in units of the model (inf: an error where the model allows none)"""
    excess = max(float(err) - floor, 0.0)
    if excess == 0.0:
        return 0.0
    return excess / model if model > 0 else math.inf


class Worst:
    """the largest ratio per observable, and where"""

    def __init__(self):
        self.rows = {}

    def add(self, what, r, where):
        if what not in self.rows or r > self.rows[what][0]:
            self.rows[what] = (r, where)

    def merge(self, other):
        for k, (r, w) in other.rows.items():
            self.add(k, r, w)

    def report(self, title):
        for k, (r, w) in sorted(self.rows.items()):
            print(f"{title} | {k} | {r:.3f} | {w}")

    def check(self):
        bad = {k: v for k, v in self.rows.items() if not v[0] <= MARGIN}
        assert not bad, bad


# ---- scenes and the device --------------------------------------------------------------------------------------------------------
def _params(precision, dt, name="default", **kw):
    over = dict(F.PARAM_SETS[name])
    over.update(kw)
    return default_params(sim_time=dt, sim_granularity=dt, precision=precision, **SOCIAL_ONLY, **over)


def _scorer(hip_mod, p, form=None):
    g = hip_mod.HipScorer(p)
    g.set_costmap(np.zeros((64, 64), dtype=np.uint8), -128.0, -128.0, 4.0)
    g.set_footprint(np.zeros((0, 2)))
    if form is not None:
        g.set_k2_form(form)
    g.set_terms_capture(True)
    return g


def _capture(g, agents, points, motion):
    g.set_agents(agents, points if len(points) else None)
    rs = (agents[0].x, agents[0].y, 0.0, motion[0], motion[1], 0.0)
    d = g.score_one_crowd(rs, 0.5, 0.0, 0.25, GOAL_ARGS)
    assert d["n_steps"] == 1 and d["cost"] >= 0, (d["n_steps"], d["cost"])
    return d, rs


MOTIONS = [(1.5, 0.75), (-1.5, 0.75), (0.75, -1.5), (-0.75, -1.5), (3.0, 2.0), (-3.0, -2.0)]


def _motion_for(agents, fr, dt):
    """a robot velocity whose step ends at least 0.75 m from where every person will be (the contact radius is 0.35)"""
    after = [(ag.x + (ag.vx + float(f.fx) * dt) * dt, ag.y + (ag.vy + float(f.fy) * dt) * dt) for ag, f in zip(agents[1:], fr[1:])]
    for mx, my in MOTIONS:
        rx, ry = agents[0].x + mx * dt, agents[0].y + my * dt
        if all(math.hypot(rx - x, ry - y) >= 0.75 for x, y in after):
            return (mx, my)
    raise AssertionError("no robot step keeps clear of the people")


def row0(m, p, agents, points, dt, dev, fr, label, worst, work_only_robot=False):
    """every entry of row 0 of a one-step capture against the mpmath forces `fr` at the handed-over state"""
    A = len(agents)
    state, work = dev["state"][0], dev["work"][0]
    assert np.all(np.isfinite(state)) and np.all(np.isfinite(work)) and np.all(work >= 0)
    robot_after = tuple(float(v) for v in state[0])
    h = mp.mpf(dt)
    for a in range(1, A):
        f, ag = fr[a], agents[a]
        model = force_model(m, p, agents, a, f)
        speed = math.hypot(state[a][2], state[a][3])
        assert speed < ag.desired_velocity  # the speed clamp did not act
        for c in (0, 1):
            vref = mp.mpf((ag.vx, ag.vy)[c]) + (f.fx, f.fy)[c] * h
            err = abs(mp.mpf(float(state[a][2 + c])) - vref)
            floor = (len(f.pairs) * m.floor + obstacle_floor(m, p, f.obstacle)) * dt
            worst.add("v'", ratio(err, floor, model * dt + U64 * abs(float(vref))), f"{label} person {a}")
            xref = mp.mpf((ag.x, ag.y)[c]) + mp.mpf(float(state[a][2 + c])) * h  # the Euler update from the returned velocity: one fma
            assert abs(mp.mpf(float(state[a][c])) - xref) <= U64 * abs(xref), (label, a, c)
        w = F.pair(p, tuple(float(v) for v in state[a]), robot_after)
        assert w.cw != 0 and w.d > ROBOT_RADIUS, (label, a)
        model = pair_model(m, p, w) + (m.e_rs + 4 * m.u) * float(w.norm)
        worst.add("Wp", ratio(abs(mp.mpf(float(work[a])) - w.norm), m.floor, model), f"{label} person {a}")
    f = fr[0]
    soc = mp.sqrt(f.social[0] ** 2 + f.social[1] ** 2)
    model = sum(pair_model(m, p, r) for r in f.pairs.values()) + (A + 2) * U64 * float(f.social[2]) + (m.d_rs + 4 * U64) * float(soc)
    model += obstacle_model(m, p, f.obstacle) + (m.d_rs + 4 * U64) * float(f.obstacle.norm) + U64 * float(soc + f.obstacle.norm)
    floor = len(f.pairs) * m.floor + obstacle_floor(m, p, f.obstacle) + 2 * NORM_FLOOR
    worst.add("Wr", ratio(abs(mp.mpf(float(work[0])) - (soc + f.obstacle.norm)), floor, model), label)
    return robot_after


def social_reference(m, p, agents, fr, dev):
    """(value, model, floor) of the S = 1 social term Wr + sum Wp, the people and the robot after the step as `dev` returned them"""
    state = dev["state"][0]
    robot_after = tuple(float(v) for v in state[0])
    f = fr[0]
    soc = mp.sqrt(f.social[0] ** 2 + f.social[1] ** 2)
    value = soc + f.obstacle.norm
    model = sum(pair_model(m, p, r) for r in f.pairs.values()) + (len(agents) + 2) * U64 * float(f.social[2]) + (m.d_rs + 4 * U64) * float(soc)
    model += obstacle_model(m, p, f.obstacle) + (m.d_rs + 4 * U64) * float(f.obstacle.norm)
    for a in range(1, len(agents)):
        w = F.pair(p, tuple(float(v) for v in state[a]), robot_after)
        value += w.norm
        model += pair_model(m, p, w) + (m.e_rs + 4 * m.u) * float(w.norm)
    floor = (len(agents) - 1) * (m.floor + m.floor_scoring) + obstacle_floor(m, p, f.obstacle) + 2 * NORM_FLOOR
    return value, model + (len(agents) + 2) * U64 * float(value), floor


class Forms:
    """the scoring kernels of one parameter set and mode: the 5 x 9 grid as the one-launch cycle, forced into the register form and
    into the flat form (the smallest grid there is: plan_info confirms each), and a sample list"""

    def __init__(self, hip_mod, p, monkeypatch):
        self.mp = monkeypatch
        self.lin, self.ang = syn.reference_sampler()
        self.auto, self.reg, self.flat = _scorer(hip_mod, p), _scorer(hip_mod, p, SFW_K2_REGISTER), _scorer(hip_mod, p, SFW_K2_FLAT)
        self.vx, self.vy, self.vth = np.array([0.5, 0.1, 0.7, 0.3, 0.0, 0.6, 0.2]), np.array([0.2, -0.3, 0.1, 0.25, 0.15, -0.05, 0.0]), np.array([0.2, -0.4, 0.0, 0.5, 0.1, -0.2, 0.3])

    def close(self):
        for g in (self.auto, self.reg, self.flat):
            g.close()

    def socials(self, agents, points, rs):
        """{form: (the social term of every scored sample, the capture of one of them)}"""
        out = {}
        pts = points if len(points) else None
        small = len(agents) < 64  # the one-launch kernel takes crowds of up to 63 agents
        for name, g, fused in (("cycle", self.auto, "1"), ("register", self.reg, "1"), ("flat", self.flat, "0")):
            self.mp.setenv("SFW_CYCLE_FUSED", fused)
            g.set_agents(agents, pts)
            g.score_grid(rs, self.lin, self.ang, GOAL_ARGS)
            plan = g.plan_info()
            if name == "cycle":
                assert plan["one_launch"] == (1 if small else 0), plan
            elif name == "register":
                assert plan["one_launch"] == 0 and plan["organisation"] in (SFW_ORG_REGISTER_1, SFW_ORG_REGISTER_2), plan
            else:
                assert plan["one_launch"] == 0 and plan["organisation"] == SFW_ORG_FLAT, plan
            t = g.cost_terms()[:, SFW_TERM_SOCIAL]
            assert np.sum(t >= 0) == len(t) - 1  # all but the (0, 0) sample
            out[name] = (t[t >= 0], g.grid_crowd(int(np.flatnonzero(t >= 0)[0])))
        self.mp.setenv("SFW_CYCLE_FUSED", "1")
        self.auto.score_samples(rs, self.vx, self.vth, GOAL_ARGS, vy=self.vy)
        t = self.auto.cost_terms()[:, SFW_TERM_SOCIAL]
        assert np.all(t >= 0)
        out["list"] = (t, self.auto.grid_crowd(0))
        return out

    def check(self, m, p, agents, points, rs, fr, label, worst):
        for name, (t, dev) in self.socials(agents, points, rs).items():
            assert dev["n_steps"] == 1
            value, model, floor = social_reference(m, p, agents, fr, dev)
            err = max(abs(mp.mpf(float(v)) - value) for v in (t.min(), t.max()))
            worst.add(f"social term, {name}", ratio(err, floor, model), label)


# ---- pair term, one person ----------------------------------------------------------------------------------------------------------
PAIR_COUNTS = {"default": 500, "wide": 200, "near": 200}
N_SCORED = 200  # of the one-person cases also go through the scoring kernels


def one_person_cases(p, name):
    """(dx, dy, wx, wy, kind) — kind "bound": held to the model; "zero": |I| down to 2^-19, where the force is below 2^-1000"""
    rng = np.random.default_rng(11)
    cases = [c + ("bound",) for c in F.pair_cases(p, PAIR_COUNTS[name], seed=3) + F.exact_fold_cases(p)]
    # the smallest |w x diff| a grid pair can have, 2^-40, both signs: theta = +-2^-29 at d = 2^-10, +-2^-41 at d = 1
    for d in (2.0 ** -10, 1.0):
        for s in (1.0, -1.0):
            cases.append((d, s * F.GRID, d + F.GRID, s * F.GRID, "bound"))
            assert cases[-1][2] * cases[-1][1] - cases[-1][3] * cases[-1][0] == s * 2.0 ** -40
    # d from 2^-10 to where the result underflows; exponents across the clamp of log2 Fs - x_d log2 e at -1100
    for d in [2.0 ** -10, 2.0 ** -8, 2.0 ** -6, 2.0 ** -3, 16.0, 40.0, 100.0, 250.0, 1000.0]:
        for _ in range(6):
            c = F.pair_from_polar(p, d, rng.uniform(-math.pi, math.pi), rng.uniform(0.2, 4.0), rng.uniform(-math.pi, math.pi))
            if c[2] * c[1] - c[3] * c[0] != 0.0:
                cases.append(c + ("bound",))
    for e in (900.0, 1000.0, 1070.0, 1099.0, 1101.0, 1150.0, 1300.0):
        for il in (0.25, 1.0):
            d = (e + math.log2(p.sfm_force_factor_social)) * math.log(2.0) * p.sfm_gamma * il
            c = F.pair_from_polar(p, d, rng.uniform(-math.pi, math.pi), il, rng.uniform(-3.0, 3.0))
            if c[2] * c[1] - c[3] * c[0] != 0.0:
                cases.append(c + ("bound",))
    for d in (0.25, 1.0, 5.0):
        for k in (1, 2, 8, 128):
            for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                ix, iy = sx * k * 2.0 ** -19, sy * k * 2.0 ** -19
                cases.append((d, 0.0, (ix - 1.0) / p.sfm_lambda, iy / p.sfm_lambda, "zero"))
                cases.append((0.0, -d, ix / p.sfm_lambda, (iy + 1.0) / p.sfm_lambda, "zero"))
    return cases


_PAIR_REFS = {}


def pair_refs(name):
    """the cases of a parameter set with the mpmath force on the person at the handed-over state, computed once (read-only)"""
    if name not in _PAIR_REFS:
        p = default_params(**F.PARAM_SETS[name])
        rng = np.random.default_rng(12)
        out = []
        for dx, dy, wx, wy, kind in one_person_cases(p, name):
            x0, y0 = (F.on_grid(v) for v in rng.uniform(-4.0, 4.0, 2))
            agents = F.agent_array([F.agent(x0, y0, wx, wy, desired_velocity=0.75), F.agent(x0 + dx, y0 + dy, desired_velocity=4096.0)])
            assert F.all_pairs_turn(agents)
            out.append((agents, F.forces(p, agents, []), kind))
        _PAIR_REFS[name] = out
    return _PAIR_REFS[name]


def measure_pairs(hip_mod, precision, monkeypatch):
    m, worst, dt = Mode(precision), Worst(), 1.0
    seen = {"bound": 0, "zero": 0, "underflow": 0, "cw+": 0, "cw-": 0, "scored": 0}
    for name in F.PARAM_SETS:
        p = _params(precision, dt, name)
        g, forms = _scorer(hip_mod, p), Forms(hip_mod, p, monkeypatch)
        refs = pair_refs(name)
        stride = max(1, len(refs) * len(F.PARAM_SETS) // N_SCORED)
        for i, (agents, fr, kind) in enumerate(refs):
            label = f"{name} #{i} diff ({agents[1].x - agents[0].x!r}, {agents[1].y - agents[0].y!r}) w ({agents[0].vx!r}, {agents[0].vy!r})"
            motion = _motion_for(agents, fr, dt)
            dev, rs = _capture(g, agents, [], motion)
            f = fr[1].pairs[0]
            seen["cw+" if f.cw > 0 else "cw-"] += 1
            seen[kind] += 1
            if kind == "zero":  # a zero, not a NaN
                assert f.norm < mp.mpf(2) ** -1000
                assert np.all(np.isfinite(dev["state"])) and abs(dev["state"][0, 1, 2]) <= 2.0 ** -1000 and abs(dev["state"][0, 1, 3]) <= 2.0 ** -1000, label
                assert 0 <= dev["work"][0, 0] <= 2.0 ** -1000, label
            seen["underflow"] += f.norm < mp.mpf(2) ** -1021
            row0(m, p, agents, [], dt, dev, fr, label, worst)
            if i % stride == 0:
                seen["scored"] += 1
                forms.check(m, p, agents, [], rs, fr, label, worst)
        g.close()
        forms.close()
    return worst, seen


@pytest.mark.parametrize("precision", PRECISIONS, ids=lambda q: MODE_NAME[q].replace(" ", "_"))
def test_pair_term_one_person(hip_mod, monkeypatch, precision):
    """~1500 one-person scenes in three parameter sets: the resting person's v' (dt = 1: the force vector itself), the robot's work
    and the person's work from the capture; every ~7th scene also through the four scoring kernels"""
    worst, seen = measure_pairs(hip_mod, precision, monkeypatch)
    worst.report(MODE_NAME[precision])
    print(seen)
    assert seen["bound"] >= 1200 and seen["zero"] >= 250 and seen["underflow"] >= 20 and seen["scored"] >= 180
    assert min(seen["cw+"], seen["cw-"]) >= 500
    worst.check()


# ---- laser points -------------------------------------------------------------------------------------------------------------------
OBSTACLE_COUNTS = [1, 15, 16, 17, 31, 32, 33, 240]  # around the boundaries of the sixteen segments of the sum


def obstacle_scenes():
    """(label, agents, points): the robot alone and with one person 40 m away, points on the grid around both — each agent sees
    near points and, at exponents of a few hundred, the other's — for every count; then the special sets"""
    rng = np.random.default_rng(21)
    robot = F.agent(0.25, -0.5, 0.40625, 0.03125, desired_velocity=0.75)
    far = F.agent(40.25, 11.5)

    def around(c, n, lo, hi):
        r, a = rng.uniform(lo, hi, n), rng.uniform(-math.pi, math.pi, n)
        return [(F.on_grid(c[0] + r[i] * math.cos(a[i])), F.on_grid(c[1] + r[i] * math.sin(a[i]))) for i in range(n)]
    out = []
    for n in OBSTACLE_COUNTS:
        out.append((f"alone, {n} points", [robot], around((robot.x, robot.y), n, 0.5, 3.0)))
        pts = around((robot.x, robot.y), (n + 1) // 2, 0.5, 3.0) + around((far.x, far.y), n // 2, 0.5, 3.0)
        order = rng.permutation(n)
        out.append((f"far person, {n} points", [robot, far], [pts[i] for i in order]))
    out.append(("a point on the robot", [robot], [(robot.x, robot.y)]))
    out.append(("points on both agents among others", [robot, far], [(robot.x, robot.y), (far.x, far.y)] + around((far.x, far.y), 5, 0.5, 2.0)))
    out.append(("points inside the radius", [robot, far], around((robot.x, robot.y), 9, 2.0 ** -6, 0.375) + around((far.x, far.y), 8, 2.0 ** -6, 0.375)))
    out.append(("points too far to count", [robot], around((robot.x, robot.y), 17, 400.0, 1500.0)))
    ring = [(robot.x + sx * a, robot.y + sy * b) for a, b in ((1.0, 0.5), (0.25, 1.75), (2.0, 2.0)) for sx in (1, -1) for sy in (1, -1)]
    out.append(("a ring whose sum cancels", [robot], ring))
    return [(label, F.agent_array(ag), np.array(pts, dtype=np.float64)) for label, ag, pts in out]


_OBSTACLE_REFS = {}


def obstacle_refs(name):
    if name not in _OBSTACLE_REFS:
        p = default_params(**F.PARAM_SETS[name])
        _OBSTACLE_REFS[name] = [(label, ag, pts, F.forces(p, ag, pts)) for label, ag, pts in obstacle_scenes() if F.all_pairs_turn(ag)]
        assert len(_OBSTACLE_REFS[name]) == 2 * len(OBSTACLE_COUNTS) + 5
    return _OBSTACLE_REFS[name]


def measure_obstacles(hip_mod, precision, monkeypatch):
    m, worst, dt = Mode(precision), Worst(), 2.0 ** -5
    for name in F.PARAM_SETS:
        p = _params(precision, dt, name)
        g, forms = _scorer(hip_mod, p), Forms(hip_mod, p, monkeypatch)
        for label, agents, points, fr in obstacle_refs(name):
            label = f"{name}: {label}"
            dev, rs = _capture(g, agents, points, _motion_for(agents, fr, dt))
            row0(m, p, agents, points, dt, dev, fr, label, worst)
            if "a point on the robot" in label:
                assert dev["work"][0, 0] == 0.0  # the term of a coincident point is exactly 0
            if "too far" in label:
                assert dev["work"][0, 0] <= 2.0 ** -1000
            if "cancels" in label:
                assert fr[0].obstacle.norm < mp.mpf(2) ** -150 * fr[0].obstacle.sum_abs  # held relative to sum |term|
            forms.check(m, p, agents, points, rs, fr, label, worst)
        g.close()
        forms.close()
    return worst


@pytest.mark.parametrize("precision", PRECISIONS, ids=lambda q: MODE_NAME[q].replace(" ", "_"))
def test_laser_point_term(hip_mod, monkeypatch, precision):
    """the mean over the laser points: the robot's work (the per-step pass, lane and task forms) and a resting person's v' (the
    starting force), three sets of sigma and k_obs; also through the scoring kernels"""
    worst = measure_obstacles(hip_mod, precision, monkeypatch)
    worst.report(MODE_NAME[precision])
    worst.check()


GLOBAL_COUNTS = [17, 31, 33]  # scan lengths that are (17, 31) and are not (33) a whole number of segments plus a shorter one


def measure_global_points(hip_mod, precision, monkeypatch):
    """A GPU-FILLING launch reads the laser points from global memory, not from the wave's LDS copy: 48 x 48 samples, more than
    eight waves per compute unit, no shared prefix (every sample makes the same step here and would be one class), forced into
    the flat form — and, for comparison, into the register form.  The capture reads them from global memory as well."""
    monkeypatch.setenv("SFW_PREFIX", "0")  # (read when a handle is created)
    monkeypatch.setenv("SFW_CYCLE_FUSED", "0")
    m, worst, dt = Mode(precision), Worst(), 2.0 ** -5
    lin, ang = syn.generalised_sampler(48, 48)  # an even number of angular samples: no (0, 0) sample
    for name in ("default", "near"):
        p = _params(precision, dt, name)
        scorers = {"flat": _scorer(hip_mod, p, SFW_K2_FLAT), "register": _scorer(hip_mod, p, SFW_K2_REGISTER)}
        for label, agents, points, fr in obstacle_refs(name):
            if not any(label.endswith(f", {n} points") for n in GLOBAL_COUNTS):
                continue
            motion = _motion_for(agents, fr, dt)
            rs = (agents[0].x, agents[0].y, 0.0, motion[0], motion[1], 0.0)
            for form, g in scorers.items():
                g.set_agents(agents, points)
                g.score_grid(rs, lin, ang, GOAL_ARGS)
                plan = g.plan_info()
                assert plan["samples"] == 48 * 48 and plan["one_launch"] == 0 and plan["levels"] == 0 and plan["chunks"] == 1, plan
                assert plan["organisation"] == (SFW_ORG_FLAT if form == "flat" else SFW_ORG_REGISTER_1), plan
                t = g.cost_terms()[:, SFW_TERM_SOCIAL]
                assert np.all(t >= 0)
                dev = g.grid_crowd(0)
                row0(m, p, agents, points, dt, dev, fr, f"{name}: {label}", worst)
                value, model, floor = social_reference(m, p, agents, fr, dev)
                err = max(abs(mp.mpf(float(v)) - value) for v in (t.min(), t.max()))
                worst.add(f"social term, {form}, 48 x 48", ratio(err, floor, model), f"{name}: {label}")
        for g in scorers.values():
            g.close()
    return worst


@pytest.mark.parametrize("precision", PRECISIONS, ids=lambda q: MODE_NAME[q].replace(" ", "_"))
def test_laser_points_in_global_memory(hip_mod, monkeypatch, precision):
    """O = 17, 31, 33, robot alone and with a far person, in a launch that fills the GPU: the flat form's loop over points in
    global memory (its second run, where the scan length is no multiple of the segment length) against the same references"""
    worst = measure_global_points(hip_mod, precision, monkeypatch)
    worst.report(MODE_NAME[precision])
    assert len([k for k in worst.rows if k.startswith("social term")]) == 2
    worst.check()


# ---- desired and group force: the pair term switched off (Fs = 0 is exactly 0 on every path) ----------------------------------------
def desired_scenes():
    """a walking person with a goal in each octant, just outside / just inside its goal radius, and without a goal"""
    robot = F.agent(-20.0, -24.0, 0.40625, 0.03125, desired_velocity=0.75)
    out = []
    for k in range(8):
        a = (k + 0.37) * math.pi / 4
        out.append((f"goal in octant {k}", F.agent(1.5, -0.75, 0.3125, -0.46875, goal=(1.5 + F.on_grid(2.0 * math.cos(a)), -0.75 + F.on_grid(2.0 * math.sin(a))))))
    for name, off in (("just outside", F.GRID), ("just inside", -F.GRID)):
        out.append((f"{name} the goal radius", F.agent(1.5, -0.75, 0.3125, -0.46875, goal=(1.5, -0.75 + 0.25 + off), goal_radius=0.25)))
    out.append(("no goal", F.agent(1.5, -0.75, 0.3125, -0.46875)))
    return [(label, F.agent_array([robot, person])) for label, person in out]


def _step_for(agents, fr):
    """the largest power of two (at most 2^-5) that keeps every person's speed after the step below 0.9 of its desired velocity"""
    dt = 2.0 ** -5
    while any(math.hypot(ag.vx, ag.vy) + math.hypot(float(f.fx), float(f.fy)) * dt >= 0.9 * ag.desired_velocity for ag, f in zip(agents[1:], fr[1:])):
        dt /= 2.0
    assert dt >= 2.0 ** -20
    return dt


def measure_desired_and_groups(hip_mod, precision, what):
    m, worst = Mode(precision), Worst()
    seen = {"gaze": 0, "no gaze": 0, "repulsion": 0, "towards": 0, "rest": 0, "x_c": set()}
    for name in ("default", "wide"):
        g = _scorer(hip_mod, _params(precision, 2.0 ** -5, name, sfm_force_factor_social=0.0))
        scenes = desired_scenes() if what == "desired" else list(F.group_scenes().items())
        for label, agents in scenes:
            assert F.all_pairs_turn(agents)
            fr = F.forces(default_params(**dict(F.PARAM_SETS[name], sfm_force_factor_social=0.0)), agents, [])
            dt = _step_for(agents, fr)
            p = _params(precision, dt, name, sfm_force_factor_social=0.0)
            g.set_params(p)
            dev, _ = _capture(g, agents, [], (0.5, 0.25))
            assert np.all(dev["work"] == 0.0)
            row0(m, p, agents, [], dt, dev, fr, f"{name}: {label}", worst)
            for f in fr[1:]:
                seen["towards" if f.desired.dir != (0, 0) else "rest"] += 1
                if f.group.n >= 2:
                    seen["gaze" if f.group.ep < 0 else "no gaze"] += 1
                    seen["repulsion"] += f.group.rep != (0, 0)
                    seen["x_c"].add(float(f.group.x_c))
        g.close()
    return worst, seen


@pytest.mark.parametrize("precision", PRECISIONS, ids=lambda q: MODE_NAME[q].replace(" ", "_"))
def test_desired_force(hip_mod, precision):
    worst, seen = measure_desired_and_groups(hip_mod, precision, "desired")
    worst.report(MODE_NAME[precision])
    assert seen["towards"] == 2 * 9 and seen["rest"] == 2 * 2 and not seen["x_c"]
    worst.check()


@pytest.mark.parametrize("precision", PRECISIONS, ids=lambda q: MODE_NAME[q].replace(" ", "_"))
def test_group_force(hip_mod, precision):
    """groups of 2, 3, 5, 8 and 82: gaze on both sides of dir . rel = 0, coherence at |centre - p| - (n - 1)/2 = -40, -1, 0, 1, 40,
    400, repulsion on both sides of the sum of the radii"""
    worst, seen = measure_desired_and_groups(hip_mod, precision, "group")
    worst.report(MODE_NAME[precision])
    print(seen)
    assert seen["gaze"] and seen["no gaze"] and seen["repulsion"] and seen["rest"]
    assert {-40.0, -1.0, 0.0, 1.0, 40.0, 400.0} <= seen["x_c"]  # |centre - p| - (n - 1)/2 at the values the scenes are built for
    worst.check()


# ---- everything at once -------------------------------------------------------------------------------------------------------------
MIXED = [(2, 240), (22, 33), (69, 17)]  # (agents, laser points); <= 4000 mpmath evaluations each: 2346 pairs + 1173 points + 68
_MIXED_REFS = {}


def mixed_refs(n_agents, n_points):
    if (n_agents, n_points) not in _MIXED_REFS:
        agents, points = F.mixed_scene(n_agents, n_points, seed=n_agents, desired_velocity=4.0)
        _MIXED_REFS[(n_agents, n_points)] = (agents, points, F.forces(default_params(), agents, points))
    return _MIXED_REFS[(n_agents, n_points)]


def measure_mixed(hip_mod, precision, monkeypatch, n_agents, n_points):
    m, worst, dt = Mode(precision), Worst(), 2.0 ** -5
    p = _params(precision, dt)
    agents, points, fr = mixed_refs(n_agents, n_points)
    g, forms = _scorer(hip_mod, p), Forms(hip_mod, p, monkeypatch)
    label = f"{n_agents} agents, {n_points} points"
    dev, rs = _capture(g, agents, points, _motion_for(agents, fr, dt))
    row0(m, p, agents, points, dt, dev, fr, label, worst)
    forms.check(m, p, agents, points, rs, fr, label, worst)
    g.close()
    forms.close()
    return worst


@pytest.mark.parametrize("precision", PRECISIONS, ids=lambda q: MODE_NAME[q].replace(" ", "_"))
@pytest.mark.parametrize("n_agents, n_points", MIXED)
def test_mixed_scene(hip_mod, monkeypatch, n_agents, n_points, precision):
    """walking people with goals, a group of three, laser points: every entry of row 0 against the full mpmath sum, and the
    social term of the four scoring kernels"""
    worst = measure_mixed(hip_mod, precision, monkeypatch, n_agents, n_points)
    worst.report(MODE_NAME[precision])
    worst.check()


if __name__ == "__main__":  # the table of profiles/r20_force_terms.txt
    from social_force_window_planner_amd import planner

    patch = pytest.MonkeyPatch()
    print("mode | term | observable | worst error / model (asserted: <= 2) | where")
    for q in PRECISIONS:
        for title, fn in (("pair term", lambda: measure_pairs(planner, q, patch)[0]), ("laser points", lambda: measure_obstacles(planner, q, patch)),
                          ("laser points, global memory", lambda: measure_global_points(planner, q, patch)),
                          ("desired force", lambda: measure_desired_and_groups(planner, q, "desired")[0]),
                          ("group force", lambda: measure_desired_and_groups(planner, q, "group")[0])):
            fn().report(f"{MODE_NAME[q]} | {title}")
        for n_agents, n_points in MIXED:
            measure_mixed(planner, q, patch, n_agents, n_points).report(f"{MODE_NAME[q]} | mixed {n_agents}/{n_points}")
    patch.undo()
    sys.exit(0)
