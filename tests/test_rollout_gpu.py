"""The robot's own rollout — the velocity recurrences, the heading sum, the pose sum, the holonomic term, the take-over of sequence
knots — and the three cost terms that need no pedestrian (SFW_TERM_VEL, _DISTANCE, _ANGLE), against tests/rollout_reference.py.

No agent vector (K2 adds nothing), a free map that holds every pose (a rejected sample's terms are sentinels), dt a power of two
(sim_time / S is exact, and a launch of S + 1 steps has the poses of S as a prefix: its pose S is the FINAL pose of the launch
under test).  Terms capture and points capture on.  Read from the device: the three terms (cost_terms), pose and heading before
every step (grid_points_batch), the final pose (pose S of the S + 1 launch; at dt = 0 the start pose).

Asserted BIT FOR BIT (the sign of a zero apart, rollout_reference.same_but_zero_sign): the heading of every step, the start pose,
the vel term, the distance term recomputed from the device's own final pose, the angle term wherever the verdict is decided; in
the straight-line family and for a standing robot every pose, and there no sample is left undecided.
Asserted within MARGIN = 2 x the model (the project's margin, tests/test_force_terms_gpu.py): every pose of every step, the final
pose, and the distance term against mpmath.  The largest measured error / model per family is printed (profiles/r22_rollout.txt).

Every family runs through every organisation that can take it, and which one ran is asserted from plan_info():
    small_grid, small_list      sfw_rollout_small_kernel (SFW_CYCLE_FUSED=0); a spec with knots runs the sequence form
    cycle_grid, cycle_list      the one-launch cycle kernel, likewise
    team                        sfw_rollout_team_kernel: the list tiled to 2049 samples, or S = 513
    thread                      sfw_rollout_kernel: the same with SFW_K1A_THREADS=1
    score_one                   sfw_score_one under the three unit weight vectors (the cost IS the term)
    batch                       member 0 of a sfw_batch launch beside two members of other map geometry (terms from the batch
                                kernel; a member's poses are re-integrated by sfw_grid_points_batch)
A grid organisation takes the specs that are a grid (no lateral target, one knot); small / cycle take S <= 512 — their S + 1 launch
at S = 512 is the team kernel's, whose poses must be the same bits.
Scratch edits of the kernels that these tests were seen to catch: profiles/r22_rollout.txt."""
import math

import numpy as np
import pytest

import rollout_reference as R
from sfw_test_util import _same
from social_force_window_planner_amd._abi import (SFW_COST_SKIPPED, SFW_ERR_INVALID_ARG, SFW_PRECISION_F32, SFW_PRECISION_F64,
                                                  SFW_PRECISION_F64_STRICT, SFW_TERM_ANGLE, SFW_TERM_DISTANCE, SFW_TERM_VEL, SfwAgent,
                                                  default_params)

pytestmark = pytest.mark.gpu

FAMILIES = R.families()
MARGIN = 2.0
GRID_ORGS = ["small_grid", "cycle_grid"]
LIST_ORGS = ["small_list", "cycle_list", "team", "thread"]
ORGS = GRID_ORGS + LIST_ORGS + ["score_one", "batch"]
UNIT = (dict(vel_weight=1.0), dict(distance_weight=1.0), dict(angle_weight=1.0))  # in term order


def _grid_scored(sp):
    return ~((sp.cmds[0, :, 0] == 0.0) & (sp.cmds[0, :, 2] == 0.0))  # the grid's never-scored (0, 0) sample


def _specs_for(org, specs):
    if org in GRID_ORGS or org == "batch":
        return [sp for sp in specs if sp.lin is not None and sp.S <= 512]
    if org in ("small_list", "cycle_list"):
        return [sp for sp in specs if sp.S <= 512]
    if org == "score_one":
        return [sp for sp in specs if sp.K == 1 and np.any(_grid_scored(sp))]  # (the (0, 0) command is left to the lists)
    return list(specs)


PAIRS = [(f, o) for f in FAMILIES for o in ORGS if _specs_for(o, FAMILIES[f])]


def _params(sp, extra=0, precision=SFW_PRECISION_F64, **weights):
    return default_params(sim_time=sp.sim_time + extra * sp.dt, sim_granularity=sp.sim_granularity, max_vel_x=sp.max_vel_x,
                          precision=precision, **weights)


def _load(g, sp, params, world=None):
    g.set_params(params)
    g.set_costmap(*(world if world is not None else R.free_map(sp)))
    g.set_footprint(np.zeros((1, 2)))
    g.set_agents((SfwAgent * 0)())
    g.set_terms_capture(True)
    g.set_points_capture(True)


def _score(g, monkeypatch, org, sp, extra=0, precision=SFW_PRECISION_F64):
    """one launch of `sp` with S + extra steps through `org` -> idx (the spec's sample behind every launched one), scored, terms, pts"""
    S = sp.S + extra
    monkeypatch.setenv("SFW_CYCLE_FUSED", "1" if org.startswith("cycle") else "0")
    monkeypatch.setenv("SFW_K1A_THREADS", "1" if org == "thread" else "0")
    _load(g, sp, _params(sp, extra, precision))
    ga = sp.acc + sp.goal
    idx = np.arange(sp.n)
    if org in GRID_ORGS:
        g.score_grid(sp.rs, sp.lin, sp.ang, ga)
        scored = _grid_scored(sp)
    else:
        if org in ("team", "thread") and sp.S <= 512:  # (the S + 1 launch of S = 512 too: the same samples)
            idx = np.resize(idx, 2049)
        c = sp.cmds[:, idx]
        vy = c[:, :, 1] if np.any(c[:, :, 1] != 0.0) else None
        if sp.K > 1:
            g.score_sequences(sp.rs, c[:, :, 0], c[:, :, 2], sp.knot_steps, ga, vy=vy)
        else:
            g.score_samples(sp.rs, c[0, :, 0], c[0, :, 2], ga, vy=None if vy is None else vy[0])
        scored = np.ones(len(idx), dtype=bool)
    info, m = g.plan_info(), len(idx)
    assert info["samples"] == m, info
    fused = m <= 2048 and S <= 512
    if org.startswith("cycle") and fused:
        assert m <= 1024 and info["one_launch"] == 1, (org, sp.name, info)
    elif org.startswith("small") and fused:
        assert info["one_launch"] == 0, (org, sp.name, info)
    else:  # K1a as a kernel of its own: the team kernel, or one thread per sample
        assert not fused and info["one_launch"] == 0 and info["chunks"] == 1 and (extra or org in ("team", "thread")), (org, sp.name, info)
    pts, _ = g.grid_points_batch(0, m, S)
    return R.NS(idx=idx, scored=scored, terms=g.cost_terms()[:, :3].copy(), pts=pts)


def _score_one(g, monkeypatch, sp, extra=0):
    """sfw_score_one of up to six samples of the spec, three calls each: under a unit weight vector the cost is the term"""
    monkeypatch.setenv("SFW_CYCLE_FUSED", "1")
    monkeypatch.setenv("SFW_K1A_THREADS", "0")
    S = sp.S + extra
    idx = np.flatnonzero(_grid_scored(sp))[:: max(1, sp.n // 6)][:6]
    terms, pts = np.empty((len(idx), 3)), np.empty((len(idx), S, 3))
    _load(g, sp, _params(sp, extra))
    for k, w in enumerate(UNIT):
        g.set_params(_params(sp, extra, social_weight=0.0, costmap_weight=0.0, **{**dict(vel_weight=0.0, distance_weight=0.0, angle_weight=0.0), **w}))
        for i, t in enumerate(idx):
            c = sp.cmds[0, t]
            terms[i, k], p = g.score_one(sp.rs, c[0], c[1], c[2], sp.acc + sp.goal, points_cap=S)
            assert p.shape == (S, 3), (sp.name, t, p.shape)
            pts[i] = p
    return R.NS(idx=idx, scored=np.ones(len(idx), dtype=bool), terms=terms, pts=pts)


def _batch_neighbours():
    a, b = FAMILIES["ramp"][0], FAMILIES["line"][0]
    return [(a, (np.zeros((32, 48), dtype=np.uint8), -12.0, -8.0, 0.5)), (b, (np.zeros((30, 20), dtype=np.uint8), -2.5, -3.75, 0.25))]


def _score_batch(hip_mod, monkeypatch, sp, extra=0):
    monkeypatch.setenv("SFW_CYCLE_FUSED", "1")
    monkeypatch.setenv("SFW_K1A_THREADS", "0")
    members = [(sp, None)] + _batch_neighbours()
    bs = hip_mod.BatchScorer(_params(sp, extra), 0, len(members))
    for i, (m, world) in enumerate(members):
        _load(bs.member(i), m, _params(m, extra if i == 0 else 0), world)
        bs.stage(i, m.rs, m.lin, m.ang, m.acc + m.goal)
    bs.launch()
    bs.fetch()
    desc = bs.describe()
    if sp.S + extra <= 512:
        assert desc["one_launch_members"] == len(members), desc
    h = bs.member(0)
    pts, _ = h.grid_points_batch(0, sp.n, sp.S + extra)
    out = R.NS(idx=np.arange(sp.n), scored=_grid_scored(sp), terms=h.cost_terms()[:, :3].copy(), pts=pts)
    bs.close()
    return out


def _run(hip_mod, g, monkeypatch, org, sp, precision=SFW_PRECISION_F64):
    """the launch under test and its final poses"""
    def one(extra):
        if org == "score_one":
            return _score_one(g, monkeypatch, sp, extra)
        if org == "batch":
            return _score_batch(hip_mod, monkeypatch, sp, extra)
        return _score(g, monkeypatch, org, sp, extra, precision)
    out = one(0)
    if sp.dt == 0.0:
        out.final = out.pts[:, 0, :2].copy()  # the robot stays
    else:
        more = one(1)
        assert R.same_but_zero_sign(more.pts[:, :sp.S], out.pts), (org, sp.name)  # the prefix
        out.final = more.pts[:, sp.S, :2].copy()
    return out


def _ratio(tally, key, err, bound):
    ok = bound > 0
    if np.any(ok):
        tally[key] = max(tally.get(key, 0.0), float(np.max(err[ok] / bound[ok])) * MARGIN)  # (the bounds carry the margin)


def _check(org, sp, out, tally):
    r = R.reference(sp, R.SINCOS_ULP_DEVICE, R.ATAN2_ULP_DEVICE, MARGIN)
    S, sc, what = sp.S, out.scored, (org, sp.name)
    assert out.pts.shape == (len(out.idx), S, 3) and out.terms.shape == (len(out.idx), 3), what
    assert np.all(out.terms[~sc] == SFW_COST_SKIPPED), what
    t, pts, terms, fin = out.idx[sc], out.pts[sc], out.terms[sc], out.final[sc]
    assert len(t) > 0, what
    # ---- bit for bit: headings, start pose, vel term, the distance term from the device's own final pose
    assert R.same_but_zero_sign(pts[:, :, 2], r.ex.th[:S, t].T), what
    assert _same(pts[:, 0, :2], np.broadcast_to(np.array(sp.rs[:2]), (len(t), 2))), what
    assert _same(terms[:, SFW_TERM_VEL], r.vel[t]), (what, terms[:4, SFW_TERM_VEL], r.vel[t][:4])
    assert _same(terms[:, SFW_TERM_DISTANCE], R.distance_term(sp.goal[0], sp.goal[1], fin[:, 0], fin[:, 1])), what
    # ---- within the model: every pose, the final pose, the distance term against mpmath
    hp = r.hp
    for c, (v, lo, b) in enumerate(((hp.x, hp.x_lo, r.bx), (hp.y, hp.y_lo, r.by))):
        err = np.abs((pts[:, :, c].T - v[:S, t]) - lo[:S, t])
        assert np.all(err <= b[:S, t]), (what, "xy"[c], float(np.max(err - b[:S, t])))
        _ratio(tally, "pose", err, b[:S, t])
        err = np.abs((fin[:, c] - v[S, t]) - lo[S, t])
        assert np.all(err <= b[S, t]), (what, "final " + "xy"[c])
        _ratio(tally, "pose", err, b[S, t])
    err = np.abs((terms[:, SFW_TERM_DISTANCE] - hp.d[t]) - hp.d_lo[t])
    assert np.all(err <= r.dist_bound[t]), (what, float(np.max(err - r.dist_bound[t])))
    _ratio(tally, "distance", err, r.dist_bound[t])
    # ---- the angle term: bit for bit wherever the verdict is decided
    dec = r.decided[t]
    assert _same(terms[dec, SFW_TERM_ANGLE], r.ang[t][dec]), (what, terms[dec, SFW_TERM_ANGLE][:4], r.ang[t][dec][:4])
    tally["samples"] = tally.get("samples", 0) + len(t)
    tally["left_out"] = tally.get("left_out", 0) + int(np.sum(~dec))
    # ---- the families without sincos: every pose bit for bit, no sample undecided
    if sp.line:
        line = R.straight_line_poses(S, sp.dt, sp.rs, r.ex)
        assert _same(pts[:, :, :2], line[:S, t].transpose(1, 0, 2)) and _same(fin, line[S, t]), what
        assert np.all(terms[:, SFW_TERM_ANGLE] == 0.0) and np.all(dec), what
    if sp.still:
        assert _same(pts[:, :, :2], np.broadcast_to(np.array(sp.rs[:2]), (len(t), S, 2))) and np.all(dec), what


@pytest.mark.parametrize("family,org", PAIRS)
def test_rollout_and_terms(hip_mod, monkeypatch, family, org):
    g = hip_mod.HipScorer(default_params())
    tally = {}
    for sp in _specs_for(org, FAMILIES[family]):
        _check(org, sp, _run(hip_mod, g, monkeypatch, org, sp), tally)
    g.close()
    print(f"r22 {family} {org}: error / model: pose {tally.get('pose', 0.0):.3f} distance {tally.get('distance', 0.0):.3f}; "
          f"{tally['left_out']} of {tally['samples']} samples left out")
    assert tally["left_out"] <= (0.01 * tally["samples"] if family == "general" else 0), tally


def test_one_sample_through_every_rollout_kernel(hip_mod, monkeypatch):
    """the same sequences through the small kernel, the cycle kernel, the team kernel and one thread per sample: the same bits"""
    g = hip_mod.HipScorer(default_params())
    for sp in FAMILIES["sequences"]:
        outs = [_run(hip_mod, g, monkeypatch, org, sp) for org in LIST_ORGS]
        for o in outs[1:]:
            n = sp.n
            assert _same(o.terms[:n], outs[0].terms[:n]) and _same(o.pts[:n], outs[0].pts[:n]) and _same(o.final[:n], outs[0].final[:n]), sp.name
    g.close()


MIXED = [("general", "general_0"), ("general", "general_6_vy"), ("ramp", "ramp_all"), ("ramp", "ramp_all_vy"), ("steps", "steps_17"),
         ("sequences", "seq_0_7_8_9_K4"), ("standing", "stand_behind"), ("line", "line_1")]


@pytest.mark.parametrize("org", ["small_grid", "cycle_grid", "small_list", "cycle_list", "team"])
def test_precision_modes_agree(hip_mod, monkeypatch, org):
    """the pedestrian-free half is double in all three modes: f64, f64 strict and f32 give the same bits, and those the reference asks for"""
    g = hip_mod.HipScorer(default_params())
    for family, name in MIXED:
        sp = next(s for s in FAMILIES[family] if s.name == name)
        if sp not in _specs_for(org, [sp]):
            continue
        outs = [_run(hip_mod, g, monkeypatch, org, sp, prec) for prec in (SFW_PRECISION_F64, SFW_PRECISION_F64_STRICT, SFW_PRECISION_F32)]
        for o in outs:
            _check(org, sp, o, {})
        for o in outs[1:]:
            assert _same(o.terms, outs[0].terms) and _same(o.pts, outs[0].pts) and _same(o.final, outs[0].final), (org, name)
    g.close()


# ---- what sfw_set_params and its kin refuse (include/sfw_hip.h, SFW_MAX_STEPS) ------------------------------------------------------------
G = 2.0 ** -6
REFUSED = [dict(sim_time=math.inf), dict(sim_time=math.nan), dict(sim_time=1e300), dict(sim_granularity=1e-300), dict(sim_granularity=math.inf),
           dict(sim_granularity=math.nan), dict(sim_time=(R.MAX_STEPS + 0.5) * G, sim_granularity=G), dict(sim_time=float(2 ** 31), sim_granularity=1.0),
           dict(max_vel_x=0.0), dict(max_vel_x=-0.0), dict(max_vel_x=math.inf), dict(max_vel_x=math.nan)]
ADMITTED = [dict(sim_time=R.MAX_STEPS * G, sim_granularity=G), dict(sim_time=float(np.nextafter((R.MAX_STEPS + 0.5) * G, 0.0)), sim_granularity=G),
            dict(sim_time=0.0), dict(max_vel_x=-0.7), dict(max_vel_x=5e-324)]


def _refused(fn, *a):
    with pytest.raises(Exception) as e:
        fn(*a)
    assert getattr(e.value, "status", None) == SFW_ERR_INVALID_ARG, e.value


def _probe(g, sp):
    g.score_samples(sp.rs, sp.cmds[0, :, 0], sp.cmds[0, :, 2], sp.acc + sp.goal, vy=sp.cmds[0, :, 1])
    return g.cost_terms().copy(), g.grid_points_batch(0, sp.n, sp.S)[0]


def test_planner_refuses_unusable_step_counts_and_max_vel_x(hip_mod, monkeypatch):
    sp = next(s for s in FAMILIES["ramp"] if s.name == "ramp_all_vy")
    for bad in REFUSED:
        _refused(hip_mod.HipScorer, default_params(**bad))
    g = hip_mod.HipScorer(default_params())
    _load(g, sp, _params(sp))
    before = _probe(g, sp)
    for bad in REFUSED:
        _refused(g.set_params, default_params(**bad))
        after = _probe(g, sp)  # the handle's params are what they were: the same step count, the same terms
        assert _same(after[0], before[0]) and _same(after[1], before[1]), bad
    for good in ADMITTED:
        g.set_params(default_params(**good))
    g.set_params(_params(sp))
    after = _probe(g, sp)
    assert _same(after[0], before[0]) and _same(after[1], before[1])
    g.close()
    for good in ADMITTED:
        hip_mod.HipScorer(default_params(**good)).close()
    # a negative max_vel_x is the caller's business: the term is the reference's expression
    g = hip_mod.HipScorer(default_params())
    neg = R.NS(**{**vars(sp), "max_vel_x": -0.7, "name": "ramp_all_vy_negative_max_vel_x"})
    out = _run(hip_mod, g, monkeypatch, "small_list", neg)
    _check("small_list", neg, out, {})
    assert np.all(out.terms[:, SFW_TERM_VEL] <= 0.0)
    g.close()


def test_batch_refuses_unusable_step_counts_and_max_vel_x(hip_mod, monkeypatch):
    sp = next(s for s in FAMILIES["ramp"] if s.name == "ramp_all")
    for bad in REFUSED:
        _refused(hip_mod.BatchScorer, default_params(**bad), 0, 2)
    for good in ADMITTED:
        hip_mod.BatchScorer(default_params(**good), 0, 2).close()
    bs = hip_mod.BatchScorer(_params(sp), 0, 2)
    h = bs.member(1)
    _load(h, sp, _params(sp))
    before = _probe(h, sp)
    for bad in REFUSED:
        _refused(h.set_params, default_params(**bad))
    after = _probe(h, sp)
    assert _same(after[0], before[0]) and _same(after[1], before[1])
    for good in ADMITTED:
        h.set_params(default_params(**good))
    bs.close()


def test_ensemble_refuses_unusable_step_counts_and_max_vel_x(hip_mod):
    from sfw_test_util import _group_scene, _params as _scene_params

    scene = _group_scene((3, 5, 0))
    for bad in REFUSED:
        _refused(hip_mod.EnsembleScorer, default_params(**bad), 0, 2)
    for good in ADMITTED:
        hip_mod.EnsembleScorer(default_params(**good), 0, 2).close()
    e = hip_mod.EnsembleScorer(_scene_params(), 0, 2)
    e.load_scene(scene, [(scene.agents, scene.obstacles)] * 2)
    args = (scene.robot_state, scene.linvels, scene.angvels, scene.goal_args)
    before = e.score_grid(*args)[0]
    for bad in REFUSED:
        _refused(e.set_params, default_params(**bad))
        assert _same(e.score_grid(*args)[0], before), bad  # the ensemble's params are what they were
    for good in ADMITTED:
        e.set_params(default_params(**good))
    e.close()
