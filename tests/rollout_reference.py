"""The robot's own rollout and the three cost terms that need no pedestrian, stated twice.  A plain module: no fixtures, nothing
pytest collects, no project code imported.

What this restates: reference sfw_planner.cpp :519-527 (step count, dt), sfw_planner.hpp :457-463 (computeNewVelocity), :581-588
(the Euler step with the OLD heading), :643-654 (distance, angle through the float normalizeAngle :399-407, velocity term), and the
knot take-over of sfw_sequences_stage (include/sfw_hip.h).  The kernels do the same in four hand-written organisations
(csrc/sfw_kernels.hip rollout_sample, sfw_rollout_team_kernel, the k1s_* phases; csrc/sfw_capi.hip new_velocity_host).

EXACT LAYER (numpy float64 / float32 element by element: one IEEE rounding per operation, never a fused one, vectorised over the
samples of a launch).  Everything in it is a fixed sequence of +, -, *, /, compare and fmod — no library function — so it is
asserted BIT FOR BIT:
    S, dt           num_steps / step_dt: int(sim_time / sim_granularity + 0.5), at least 1, refused beyond MAX_STEPS; sim_time / S
    velocities      new_velocity: step = a * dt; up = min(vg, vi + step); dn = max(vg, vi - step); (vg - vi) >= 0 ? up : dn
    headings        th_{i+1} = th_i + vth_i * dt with the NEW velocity; th[i] is the heading before step i, th[S] the final one
    vel             |max_vel_x - vx_{S-1}| / max_vel_x
    distance        from a given final pose: dx = wpx - x, dy = wpy - y, dx * dx + dy * dy (each product and the sum rounded)
    angle           from a given double a: float cast, then `val >= mn ? mn + fmodf(val - mn, mx - mn) : mx - fmodf(mn - val, mx - mn)`
                    in float32 with mn = float(-M_PI), mx = float(M_PI); then |.| / M_PI in double
    straight line   heading 0 throughout and no lateral velocity: cos = 1, sin = 0 exactly, so the poses are exact-layer too
Zeros: the device's fmin / fmax order -0.0 below +0.0 and numpy's compare does not, so min / max are written as a select on < / >
and a tie between the zeros may return either.  The SIGN OF A ZERO velocity is therefore not compared (same_but_zero_sign); it can
reach a pose only as the sign of a zero coordinate, and no term at all.

HIGH-PRECISION LAYER (mpmath, PREC bits).  The poses with exact sin / cos of the exact layer's headings — for the lateral term of
the exact layer's double M_PI_2 + th_i, the very argument the kernels hand to sincos — and the exact layer's velocities, nothing
rounded on the way; the squared distance and the angle atan2(wpy - y_S, wpx - x_S) - th_S of the exact final pose.  Values come
back as a double and the double's own residual (x, x_lo), so that a caller forms |device - exact| without the reference's
rounding in it.

THE MODEL (first order in u = 2^-53).  The kernels compute
    x_{i+1} = fl(x_i + fl(fl(fl(vx_i c_i) + fl(vy_i c2_i)) dt)),   c_i = cos(th_i)(1 + e), |e| <= E_sc,
the products and the sum each within u of their value, so the increment is within (|vx_i| + |vy_i|) dt (E_sc + 3u) of the exact
one (|c|, |c2| <= 1; the sum's and the dt product's roundings are relative to at most that magnitude), and the addition adds
u |x_{i+1}|.  Errors already in x_i pass through the addition unchanged.  Hence
    |x_S - X_S| <= sum_i [ (|vx_i| + |vy_i|) dt (E_sc + 3u) + u |x_{i+1}| ]                                          (pose_bound)
and the same for y.  A step whose velocities are both zero adds an exact 0 and contributes nothing, not even the u |x| term.
Below DBL_MIN a rounding is no longer relative: each of a step's four operations may be off by half the smallest subnormal,
2^-1075, whatever its result — two subnormal quanta per step that moved, added to the bound (ramp_acc_dbl_min lives there).
E_sc: the library's sin / cos error as a relative figure, k ulp = k 2^-52 (an ulp is at most 2^-52 of the value).  For the device
library the project's convention (tests/test_blend_gpu.py, tests/test_perturb_gpu.py) is the OpenCL full-profile class, 4 ulp for
sin / cos and 6 ulp for atan2; glibc's are 1 ulp.
    distance        dx = fl(wpx - x_S) is within Bx + u |dx| of the exact difference; d = fl(fl(dx dx) + fl(dy dy)):
                    |d - D| <= 2 |dx| (Bx + u |dx|) + 2 |dy| (By + u |dy|) + u dx^2 + u dy^2 + u d
                             <= 2 |dx| Bx + 2 |dy| By + 4 u d                                                        (distance_bound)
    angle           a = fl(fl(atan2(dy, dx)) - th_S); d atan2 = (dx ddy - dy ddx) / (dx^2 + dy^2):
                    |a - A| <= (|dx| (By + u |dy|) + |dy| (Bx + u |dx|)) / (dx^2 + dy^2) + E_at 2^-52 |atan2| + u |a|   (angle_bound)
                    atan2(+-0, x) is fixed by definition (C Annex F: +-0 for x > 0, the double pi for x < 0): no E_at there,
                    only u pi for the double pi, and 0 - th_S is exact.

THE ANGLE TERM'S VERDICT.  The float cast and the wrap at +-float(pi) are discontinuous, so the term has no tolerance.  If
float(A - delta) == float(A + delta) — the whole interval of the double angle rounds to ONE float, and the branch of
normalizeAngle is a function of that float — the term must equal angle_term(A) bit for bit (angle_verdict: decided).  Otherwise
the sample is left out.  A float has 2^-24 relative spacing and delta is some 1e-15, so about 1e-7 of random samples are left
out; the constructed families (delta = 0) leave out none."""
import math
from types import SimpleNamespace as NS

import mpmath as mp
import numpy as np

PREC = 200
U = 2.0 ** -53
ULP = 2.0 ** -52
SUBNORMAL = 2.0 ** -1074
MAX_STEPS = 1 << 20  # SFW_MAX_STEPS (include/sfw_hip.h)
SINCOS_ULP_DEVICE, ATAN2_ULP_DEVICE = 4.0, 6.0  # the project's convention for the device library
SINCOS_ULP_LIBM, ATAN2_ULP_LIBM = 1.0, 1.0      # glibc
F32_PI = np.float32(math.pi)
F32_NEG_PI = np.float32(-math.pi)


# ---- exact layer ------------------------------------------------------------------------------------------------------------------
def num_steps(sim_time, sim_granularity):
    """num_steps_of behind check_params (csrc/sfw_capi.hip); ValueError for what sfw_set_params refuses"""
    st, g = float(sim_time), float(sim_granularity)
    if not (math.isfinite(st) and math.isfinite(g) and g > 0 and st >= 0):
        raise ValueError("sim_time / sim_granularity out of range")
    q = st / g + 0.5
    if not q < float(MAX_STEPS) + 1.0:
        raise ValueError("more than MAX_STEPS steps")
    n = int(q)
    return 1 if n == 0 else n


def step_dt(sim_time, S):
    return float(sim_time) / S  # ref :527 (fill_launch)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def new_velocity(vg, vi, a_max, dt):
    """computeNewVelocity over arrays: both candidates, then the select on (vg - vi) >= 0"""
    with np.errstate(over="ignore"):
        step = np.float64(a_max) * np.float64(dt)  # (may overflow to inf: both candidates then lose to the target)
        up_c, dn_c = vi + step, vi - step
    up = np.where(vg < up_c, vg, up_c)
    dn = np.where(vg > dn_c, vg, dn_c)
    return np.where((vg - vi) >= 0, up, dn)


def rollout(S, dt, rs, acc, cmds, knot_steps=(0,)):
    """Velocities and headings of n samples.  rs: (x, y, theta, vx, vy, vtheta); acc: (acc_x, acc_y, acc_theta); cmds: (K, n, 3)
    targets (vx, vy, vtheta) per knot, or (n, 3) for one knot; knot_steps[k]: the step at which knot k takes over (knot_steps[0]
    == 0, strictly ascending; a knot at a step >= S is never reached).
    -> vx, vy, vth: (S, n) velocities AFTER step i's update; th: (S + 1, n) heading before step i, th[S] the final one"""
    cmds = _f64(cmds)
    if cmds.ndim == 2:
        cmds = cmds[None]
    K, n, _ = cmds.shape
    ks = [int(k) for k in knot_steps]
    assert len(ks) == K and ks[0] == 0 and all(b > a for a, b in zip(ks, ks[1:]))
    dt = np.float64(dt)
    vx, vy, vth = (np.full(n, np.float64(rs[3 + c])) for c in range(3))
    th = np.full(n, np.float64(rs[2]))
    out = NS(vx=np.empty((S, n)), vy=np.empty((S, n)), vth=np.empty((S, n)), th=np.empty((S + 1, n)))
    k = 0
    for i in range(S):
        if k + 1 < K and ks[k + 1] == i:  # the next knot takes over AT its step
            k += 1
        vx = new_velocity(cmds[k, :, 0], vx, acc[0], dt)
        vy = new_velocity(cmds[k, :, 1], vy, acc[1], dt)
        vth = new_velocity(cmds[k, :, 2], vth, acc[2], dt)
        out.vx[i], out.vy[i], out.vth[i], out.th[i] = vx, vy, vth, th
        th = th + vth * dt
    out.th[S] = th
    return out


def vel_term(max_vel_x, vx_last):
    return np.abs(np.float64(max_vel_x) - _f64(vx_last)) / np.float64(max_vel_x)


def distance_term(wpx, wpy, x, y):
    dx, dy = np.float64(wpx) - _f64(x), np.float64(wpy) - _f64(y)
    return dx * dx + dy * dy


def normalize_angle_f32(val):
    """the reference's float normalizeAngle(val, float(-M_PI), float(M_PI)) on float32 values, in float32 arithmetic"""
    val = np.asarray(val, dtype=np.float32)
    span = np.float32(F32_PI - F32_NEG_PI)
    hi = F32_NEG_PI + np.fmod(val - F32_NEG_PI, span)
    lo = F32_PI - np.fmod(F32_NEG_PI - val, span)
    out = np.where(val >= F32_NEG_PI, hi, lo)
    assert out.dtype == np.float32
    return out


def angle_term(a):
    """from the double angle atan2(dy, dx) - th_S"""
    return np.abs(normalize_angle_f32(_f64(a).astype(np.float32)).astype(np.float64)) / np.float64(math.pi)


def straight_line_poses(S, dt, rs, ex):
    """(S + 1, n, 2) poses of a rollout whose headings are all 0 and whose lateral velocity is 0 throughout: cos = 1, sin = 0,
    x_{i+1} = x_i + (vx_i * 1 + 0 * 0) * dt, y_{i+1} = y_i + (vx_i * 0 + 0 * 0) * dt — exact layer"""
    assert np.all(ex.th == 0.0) and np.all(ex.vy == 0.0)
    n = ex.vx.shape[1]
    p = np.empty((S + 1, n, 2))
    p[0, :, 0], p[0, :, 1] = rs[0], rs[1]
    for i in range(S):
        p[i + 1, :, 0] = p[i, :, 0] + (ex.vx[i] * 1.0 + ex.vy[i] * 0.0) * np.float64(dt)
        p[i + 1, :, 1] = p[i, :, 1] + (ex.vx[i] * 0.0 + ex.vy[i] * 0.0) * np.float64(dt)
    return p


def same_but_zero_sign(a, b):
    """bit for bit, shape included, except that +0.0 and -0.0 are one value (and no NaN anywhere)"""
    a, b = _f64(a), _f64(b)
    if a.shape != b.shape or np.isnan(a).any() or np.isnan(b).any():
        return False
    return bool(np.array_equal(a, b))  # value equality of non-NaN doubles IS bit equality apart from the zeros


# ---- high-precision layer -----------------------------------------------------------------------------------------------------------
def _split(v):
    hi = float(v)
    return hi, float(v - mp.mpf(hi))


def hp_rollout(S, dt, rs, goal, ex):
    """Poses, squared distance and final angle of every sample of the exact-layer rollout `ex`, in mpmath.
    -> x, y: (S + 1, n) doubles with residuals x_lo, y_lo (pose before step i; [S] the final pose); path: (S + 1, n) running
    sum_i (|vx_i| + |vy_i|) dt; moved: the steps so far with a velocity other than 0; sax, say: running sum_i |x_{i+1}|, |y_{i+1}| over the steps that moved; d, d_lo: the squared
    distance to the goal; ang, ang_lo: atan2(wpy - y_S, wpx - x_S) - th_S; at: |atan2|; dx, dy: the differences as doubles"""
    n = ex.vx.shape[1]
    o = NS(x=np.empty((S + 1, n)), y=np.empty((S + 1, n)), x_lo=np.empty((S + 1, n)), y_lo=np.empty((S + 1, n)),
           path=np.zeros((S + 1, n)), sax=np.zeros((S + 1, n)), say=np.zeros((S + 1, n)), ang=np.empty(n), ang_lo=np.empty(n),
           at=np.empty(n), dx=np.empty(n), dy=np.empty(n), d=np.empty(n), d_lo=np.empty(n), moved=np.zeros((S + 1, n)))
    cs = {}

    def cos_sin(th):
        v = cs.get(th)
        if v is None:
            v = cs[th] = mp.cos_sin(mp.mpf(th))
        return v
    with mp.workprec(PREC):
        mdt = mp.mpf(float(dt))
        for j in range(n):
            x, y = mp.mpf(float(rs[0])), mp.mpf(float(rs[1]))
            path = sax = say = mp.mpf(0)
            moved = 0
            for i in range(S):
                o.moved[i, j] = moved
                o.x[i, j], o.x_lo[i, j] = _split(x)
                o.y[i, j], o.y_lo[i, j] = _split(y)
                o.path[i, j], o.sax[i, j], o.say[i, j] = float(path), float(sax), float(say)
                vx, vy, th = float(ex.vx[i, j]), float(ex.vy[i, j]), float(ex.th[i, j])
                if vx == 0.0 and vy == 0.0:
                    continue
                c, s = cos_sin(th)
                ix, iy = mp.mpf(vx) * c, mp.mpf(vx) * s
                if vy != 0.0:
                    c2, s2 = cos_sin(math.pi / 2 + th)  # the double M_PI_2 + th_i, as the kernels form it
                    ix, iy = ix + mp.mpf(vy) * c2, iy + mp.mpf(vy) * s2
                x, y = x + ix * mdt, y + iy * mdt
                path += (abs(mp.mpf(vx)) + abs(mp.mpf(vy))) * mdt
                sax, say = sax + abs(x), say + abs(y)
                moved += 1
            o.moved[S, j] = moved
            o.x[S, j], o.x_lo[S, j] = _split(x)
            o.y[S, j], o.y_lo[S, j] = _split(y)
            o.path[S, j], o.sax[S, j], o.say[S, j] = float(path), float(sax), float(say)
            dx, dy = mp.mpf(float(goal[0])) - x, mp.mpf(float(goal[1])) - y
            at = mp.atan2(dy, dx)
            o.d[j], o.d_lo[j] = _split(dx * dx + dy * dy)
            o.ang[j], o.ang_lo[j] = _split(at - mp.mpf(float(ex.th[S, j])))
            o.at[j], o.dx[j], o.dy[j] = float(abs(at)), float(dx), float(dy)
    return o


def pose_bound(hp, sincos_ulp):
    """(Bx, By): (S + 1, n) model bounds of every pose"""
    e = sincos_ulp * ULP + 3 * U
    tiny = 2.0 * SUBNORMAL * hp.moved
    return hp.path * e + U * hp.sax + tiny, hp.path * e + U * hp.say + tiny


def distance_error(hp, d):
    """|a launch's distance terms - exact|: the difference to the double is exact, then the double's own residual"""
    return np.abs((_f64(d) - hp.d) - hp.d_lo)


def distance_bound(hp, sincos_ulp):
    bx, by = pose_bound(hp, sincos_ulp)
    return 2 * np.abs(hp.dx) * bx[-1] + 2 * np.abs(hp.dy) * by[-1] + 4 * U * hp.d


def angle_bound(hp, sincos_ulp, atan2_ulp):
    bx, by = pose_bound(hp, sincos_ulp)
    adx, ady = np.abs(hp.dx), np.abs(hp.dy)
    with np.errstate(divide="ignore", invalid="ignore"):
        prop = np.where(hp.d > 0, (adx * (by[-1] + U * ady) + ady * (bx[-1] + U * adx)) / hp.d, 0.0)
    # atan2(+-0, x) is +-0 for x > 0 and the DOUBLE pi for x < 0 by definition: no library figure, only pi's own rounding;
    # and 0 - th_S is exact
    lib = np.where(hp.dy == 0.0, U * hp.at, atan2_ulp * ULP * hp.at)
    return prop + lib + np.where(hp.at == 0.0, 0.0, U * np.abs(hp.ang))


def angle_verdict(hp, delta):
    """-> (decided, term): where the whole interval [A - delta, A + delta] casts to one float the term is angle_term(A)"""
    slack = np.where(delta > 0, delta + 2 * U * np.abs(hp.ang), 0.0)  # (forming A -+ delta in doubles rounds once more)
    lo, hi = (hp.ang - slack).astype(np.float32), (hp.ang + slack).astype(np.float32)
    return lo == hi, angle_term(hp.ang)


# ---- the case lists (tests/test_rollout_gpu.py runs them; tests/test_rollout_reference.py holds them to the oracle) -----------------
# One spec is one launch: the samples of a launch share robot state, limits, goal and knot steps and differ in their targets.
# lin / ang: the grid axes when the targets are their product with no lateral target (sample t = iv * len(ang) + iw), else None.
DT = 2.0 ** -6
Q = 1.0 * DT  # the velocity step of acc = 1
RAMP_TARGETS = np.array([0.5, 0.0, 0.25 + 3 * Q, 0.25 + 2.5 * Q, 0.7, 0.25, -0.125, -0.0])
# above / below the start velocity 0.25; reached exactly on step 3; overshot at step 3 and clipped; not reached in 20 steps
# (0.25 + 20 / 64 < 0.7); equal to the start from step 0; the other sign; -0.0


def spec(name, S, rs, acc, goal, cmds, lin=None, ang=None, knot_steps=(0,), dt=DT, max_vel_x=0.7, sim_time=None, line=False, still=False):
    cmds = _f64(cmds)
    if cmds.ndim == 2:
        cmds = cmds[None]
    return NS(name=name, S=S, dt=dt, sim_time=S * dt if sim_time is None else sim_time, sim_granularity=dt if dt > 0 else DT,
              rs=tuple(float(v) for v in rs), acc=tuple(float(v) for v in acc), goal=tuple(float(v) for v in goal), cmds=cmds,
              lin=None if lin is None else _f64(lin), ang=None if ang is None else _f64(ang), knot_steps=tuple(knot_steps),
              max_vel_x=max_vel_x, line=line, still=still, K=cmds.shape[0], n=cmds.shape[1])


def product(lin, ang, vy=None):
    """(n, 3) targets of the grid lin x ang in the grid's sample order; vy: a lateral target per sample (a list, no grid any more)"""
    lin, ang = _f64(lin), _f64(ang)
    c = np.zeros((len(lin) * len(ang), 3))
    c[:, 0], c[:, 2] = np.repeat(lin, len(ang)), np.tile(ang, len(lin))
    if vy is not None:
        c[:, 1] = np.resize(_f64(vy), len(c))
    return c


def _both(name, S, rs, acc, goal, lin, ang, vy, **kw):
    """the grid and the same grid as a list with lateral targets"""
    return [spec(name, S, rs, acc, goal, product(lin, ang), lin, ang, **kw), spec(name + "_vy", S, rs, acc, goal, product(lin, ang, vy), **kw)]


STEP_COUNTS = (1, 2, 7, 8, 9, 15, 16, 17, 40, 511, 512, 513)


def step_count_specs():
    rs, acc, goal = (0.5, -0.25, 0.3, 0.2, 0.0, 0.1), (1.0, 0.5, 1.0), (7.0, 5.0)
    lin, ang, vy = [0.0, 0.3, 0.7], [-0.5, 0.0, 0.25], [0.1, -0.2]
    out = []
    for S in STEP_COUNTS:  # (8 s at the long horizons: at most 5.6 m)
        out += _both(f"steps_{S}", S, rs, acc, goal, lin, ang, vy)
    # sim_time = 0: one step of dt = 0, the robot stays and the terms are the start pose's
    out += _both("steps_time0", 1, rs, acc, goal, lin, ang, vy, dt=0.0, sim_time=0.0)
    return out


def ramp_specs():
    T, S, goal = RAMP_TARGETS, 20, (4.0, 3.0)
    rs = (0.0, 0.0, 0.2, 0.25, 0.25, 0.25)
    one = (1.0, 1.0, 1.0)
    out = [spec("ramp_x", S, rs, one, goal, product(T, [0.0]), T, [0.0]),           # (0, 0) and (-0, 0): never scored by a grid
           spec("ramp_th", S, rs, one, goal, product([0.3], T), [0.3], T),
           spec("ramp_y", S, rs, one, goal, product([0.3], [0.0] * len(T), T))]
    out += _both("ramp_all", S, rs, one, goal, T, T, np.roll(T, 3))
    out += _both("ramp_acc0", S, rs, (0.0, 0.0, 0.0), goal, T, T, np.roll(T, 3))      # the velocity never changes
    out += _both("ramp_acc_negative", S, rs, (-1.0, -0.5, -1.0), goal, T, T, np.roll(T, 3))  # the caller's business: as the reference computes
    out += _both("ramp_acc_overflow", 3, rs, (1e308,) * 3, goal, T, T, np.roll(T, 3), dt=2.0)  # a * dt = inf
    tiny = float(np.finfo(np.float64).tiny) / DT
    out += _both("ramp_acc_dbl_min", S, (0.0, 0.0, 0.2, 0.0, 0.0, 0.0), (tiny,) * 3, goal, T, T, np.roll(T, 3))  # a * dt = DBL_MIN
    return out


def straight_line_specs():
    lin = [0.1, 0.3, 0.7, 0.0, 0.7 - 2.0 ** -40]
    out = []
    for k, (x0, y0) in enumerate([(0.0, 0.0), (1e4, 0.0), (-1e4, -1e4), (1e4 + 0.3, 0.1), (-0.7, 1e4)]):
        rs = (x0, y0, 0.0, 0.25 + 2.0 ** -30, 0.0, 0.0)
        out.append(spec(f"line_{k}", 17, rs, (1.0, 1.0, 1.0), (x0 + 8.0, y0), product(lin, [0.0]), lin, [0.0], line=True))
    return out


def standing_headings():
    f = np.float32
    pi32, m2pi32 = F32_PI, np.float32(F32_PI - F32_NEG_PI)
    around = []
    for s in (f(1), f(-1)):
        p = f(s * pi32)
        around += [float(p), float(np.nextafter(p, f(np.inf))), float(np.nextafter(p, f(-np.inf))),
                   float(np.nextafter(np.float64(p), np.inf)), float(np.nextafter(np.float64(p), -np.inf))]  # doubles that round to float(+-pi)
    return np.concatenate([np.linspace(-10 * math.pi, 10 * math.pi, 41), around, [float(f(k) * m2pi32) for k in range(-3, 4) if k],
                           [math.pi, -math.pi, 1e-300, -1e-300, 0.0]])


def standing_specs():
    """th_S = th_0 + vth * 1.0 with th_0 = 0 and an acceleration limit that every target is inside: th_S IS the target"""
    ang = standing_headings()
    acc = (1.0, 1.0, 1e300)
    out = []
    for name, goal in (("ahead", (2.5, -1.0)), ("on_goal", (0.5, -1.0)), ("behind", (-1.5, -1.0))):
        out.append(spec(f"stand_{name}", 1, (0.5, -1.0, 0.0, 0.0, 0.0, 0.0), acc, goal, product([0.0], ang), [0.0], ang, dt=1.0, still=True))
    out.append(spec("stand_negzero", 1, (0.5, -1.0, -0.0, 0.0, 0.0, -0.0), acc, (2.5, -1.0), product([0.0], [-0.0, 0.0]), dt=1.0, still=True))  # (a list: a grid never scores (0, 0))
    return out


def general_specs():
    """2048 random samples with and without a lateral target: eight start headings of 16 x 16 targets each"""
    rng = np.random.default_rng(22)
    heads = list(rng.uniform(-math.pi, math.pi, 4)) + [1e3, -1e6, math.pi - 0.05, -math.pi + 0.02]
    out = []
    for k, th0 in enumerate(heads):
        lin, ang = rng.uniform(0.0, 0.7, 16), rng.uniform(-0.5, 0.5, 16)
        if k == 6:
            ang = np.abs(ang) + 0.3  # crosses +pi inside the horizon
        if k == 7:
            ang = -np.abs(ang) - 0.2  # crosses -pi
        x0, y0 = rng.uniform(-3, 3, 2)
        rs = (x0, y0, th0, rng.uniform(0, 0.5), rng.uniform(-0.1, 0.1), rng.uniform(-0.3, 0.3))
        out += _both(f"general_{k}", 9, rs, (1.0, 0.7, 1.3), (x0 + 3.0, y0 - 2.0), lin, ang, rng.uniform(-0.3, 0.3, 256), dt=2.0 ** -5)
    return out


SEQ_S = 20
SEQ_KNOTS = [(0,), (0, 1), (0, 7, 8, 9), (0, 8, SEQ_S - 1), (0, SEQ_S, SEQ_S + 5), (0, 3, 4), tuple(range(64))]
# K = 1, 2, 3, 64; knots at 0 and 1; at 7, 8, 9 — CYCLE_HEAD = 8 is the one step at which the cycle kernels resume the phases
# (csrc/sfw_kernels.hip cycle_block), so that step and its neighbours; at S - 1; at S and beyond (ignored); adjacent steps


def sequence_specs():
    rng = np.random.default_rng(23)
    rs, acc, goal, n = (0.2, 0.1, -0.4, 0.3, 0.05, -0.1), (1.0, 0.7, 1.3), (3.0, -2.5), 16
    out = []
    for ks in SEQ_KNOTS:
        K = len(ks)
        cmds = np.stack([rng.uniform(0.0, 0.7, (K, n)), rng.uniform(-0.3, 0.3, (K, n)), rng.uniform(-0.5, 0.5, (K, n))], axis=2)
        out.append(spec("seq_" + "_".join(str(k) for k in ks[:4]) + f"_K{K}", SEQ_S, rs, acc, goal, cmds, knot_steps=ks))
    # a knot whose target equals the running velocity: knot 1 at step 5 asks for what step 4 left
    cmds = np.stack([rng.uniform(0.0, 0.7, (3, n)), rng.uniform(-0.3, 0.3, (3, n)), rng.uniform(-0.5, 0.5, (3, n))], axis=2)
    ex = rollout(SEQ_S, DT, rs, acc, cmds[:1])
    cmds[1, :, 0], cmds[1, :, 1], cmds[1, :, 2] = ex.vx[4], ex.vy[4], ex.vth[4]
    out.append(spec("seq_running", SEQ_S, rs, acc, goal, cmds, knot_steps=(0, 5, 12)))
    return out


def families():
    return {"steps": step_count_specs(), "ramp": ramp_specs(), "line": straight_line_specs(), "standing": standing_specs(),
            "general": general_specs(), "sequences": sequence_specs()}


_REF = {}


def reference(sp, sincos_ulp, atan2_ulp, margin=1.0):
    """Both layers of a spec, computed once and shared (never written to): ex, hp; vel, the exact vel term; bx, by: pose bounds
    times margin; dist_bound; decided, ang: the angle term's verdict under margin * angle_bound"""
    key = (sp.name, sincos_ulp, atan2_ulp, margin)
    if key not in _REF:
        ex = rollout(sp.S, sp.dt, sp.rs, sp.acc, sp.cmds, sp.knot_steps)
        hp = hp_rollout(sp.S, sp.dt, sp.rs, sp.goal, ex)
        bx, by = pose_bound(hp, sincos_ulp)
        decided, ang = angle_verdict(hp, margin * angle_bound(hp, sincos_ulp, atan2_ulp))
        if sp.still or sp.line:
            # the position is exact and the goal lies on the robot's world x axis: atan2(+0, dx) is +0 for dx >= 0 and the double
            # pi for dx < 0 by definition (C Annex F), so the double angle is exact-layer too and every sample is decided
            # (a line spec moves along +x by less than its goal's 8 m lead: dx > 0 whatever the roundings of x)
            dx, dy = np.float64(sp.goal[0]) - np.float64(sp.rs[0]), np.float64(sp.goal[1]) - np.float64(sp.rs[1])
            assert dy == 0.0 and np.all(hp.y[-1] == sp.rs[1]) and (sp.still or (dx == 8.0 and np.all(hp.path[-1] < 1.0)))
            ang = angle_term(np.where(dx >= 0, 0.0, math.pi) - ex.th[sp.S])
            decided = np.ones(sp.n, dtype=bool)
        _REF[key] = NS(ex=ex, hp=hp, vel=vel_term(sp.max_vel_x, ex.vx[sp.S - 1]), bx=margin * bx, by=margin * by,
                       dist_bound=margin * distance_bound(hp, sincos_ulp), decided=decided, ang=ang)
    return _REF[key]


def free_map(sp):
    """a free 64 x 64 map of 1 m cells around the start pose: it holds every pose of every spec (the robot moves 6 m at most)"""
    return np.zeros((64, 64), dtype=np.uint8), float(round(sp.rs[0])) - 32.0, float(round(sp.rs[1])) - 32.0, 1.0
