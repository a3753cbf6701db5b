"""The device math of csrc/sfw_math.h on the device, function by function, against high-precision references
(tests/probe/sfw_math_probe.hip: one element-wise kernel per function; both builds: the default polynomial degrees and the
strict K2 build's asin 8 / exp 9).  The rollout tests see these functions only through whole costs held to 1e-9; a wrong
coefficient digit, a Newton step whose halving did not act or a fold that flips at y == |x| moves a force term from 1e-14 to
1e-11 or 1e-7 and passes all of them.

References (tests/device_math_util.py): mpmath at the exact inputs for every listed edge and 3000 random elements, np.longdouble
for the bulk, the two asserted to agree to 1e-18.  Every asserted number is
  * a figure quoted from sfw_math.h with its margin (exp2: 1.25 x the table's; angle: 1.25 x the table's + 4 ulp(pi)),
  * one of the caps 2.2e-14 (root) / 1.5e-14 (reciprocal) / 1e-6 (f32), or
  * twice a value measured against mpmath on an MI355X, rounded up to a power of two (MEASURED below = the rows of
    profiles/r18_device_math.txt, which `python tests/test_device_math_gpu.py` prints).
None is taken from the device code's own output; the bit-identity checks compare the library with itself on purpose."""
import sys

import numpy as np
import pytest

import device_math_util as U

pytestmark = pytest.mark.gpu

BUILDS = ("default", "strict")
# worst errors measured on an MI355X against the references above (profiles/r18_device_math.txt); the same in both builds
MEASURED = {
    "rsqrt": 3.897e-15, "sqrt": 3.945e-15, "rcp_nr": 2.128e-15,
    "rsqrt f32": 9.119e-8, "sqrt f32": 1.175e-7, "rcp_nr f32": 8.869e-8, "exp2_fast f32": 8.140e-8, "exp2_scaled f32": 8.094e-8,
    "exp2_scaled f32, exact product, |u c| <= 16": 3.853e-7, "angle_abs f32": 3.020e-7,
}
F32_SCALED_EXACT_RANGE = 16.0  # exp2_scaled(float) rounds u c to float first: 2^-24 |u c| ln 2 of the result, 6.6e-7 at 16


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


class Inputs:
    """the input sets and their references, computed once per module (the references are read-only)"""

    def __init__(self, dtype):
        self.dtype = dtype
        f32 = dtype == np.float32
        self.x, self.x_edge = U.exp2_inputs(dtype)
        self.x_ref = U.exp2_reference("2^x", self.x, np.zeros(len(self.x)), self.x_edge)
        self.u, self.c, self.uc_edge = U.exp2_scaled_inputs(dtype)
        if f32:  # the product of two floats is exact in f64; the function itself rounds it to float
            self.uc, lo = self.u.astype(np.float64) * self.c.astype(np.float64), np.zeros(len(self.u))
            self.uc_rounded = (self.u * self.c).astype(np.float64)
            self.uc_rounded_ref = U.exp2_reference("2^fl(u c)", self.uc_rounded, lo, self.uc_edge)
        else:
            self.uc, lo = U.two_product(self.u, self.c)
        self.uc_ref = U.exp2_reference("2^(u c)", self.uc, lo, self.uc_edge)
        self.r, self.r_edge = U.root_inputs(dtype)
        self.rs_ref, self.sq_ref = U.root_references(self.r, self.r_edge)
        self.q, self.q_edge = U.rcp_inputs(dtype)
        self.q_ref = U.rcp_reference(self.q, self.q_edge)
        self.ay, self.ax, self.a_edge, self.folds, self.a_exact = U.angle_inputs(dtype)
        self.a_ref, self.rh, self.hyp = U.angle_reference(self.ay, self.ax, self.a_edge)
        self.theta0 = int(np.flatnonzero((self.ay[:self.a_exact] == 0) & (self.ax[:self.a_exact] == 1.0))[0])
        h = np.hypot(self.ax.astype(np.float64), self.ay.astype(np.float64))
        self.composable = (h > 1e-100) & (h < 1e100)  # nx^2 + y^2 neither under- nor overflows


class Run:
    """every probe kernel of one build run once on the module's inputs"""

    def __init__(self, probe, i64, i32):
        self.probe = probe
        for tag, i, t in (("", i64, np.float64), ("_f32", i32, np.float32)):
            setattr(self, "exp2" + tag, probe.exp2_fast(i.x, dtype=t))
            setattr(self, "scaled" + tag, probe.exp2_scaled(i.u, i.c, dtype=t))
            rs, sq = probe.rsqrt_sqrt(i.r, dtype=t)
            setattr(self, "rs" + tag, rs)
            setattr(self, "sq" + tag, sq)
            setattr(self, "rcp" + tag, probe.rcp_nr(i.q, dtype=t))
            setattr(self, "angle" + tag, probe.angle_abs(i.ay, -i.ax, i.rh, i.hyp, dtype=t))
        self.composed = probe.angle_abs_composed(i64.ay[i64.composable], -i64.ax[i64.composable])


def figures(run, i64, i32):
    """{function: (worst error, bound or None while unmeasured, where, violated rules)} of one build — the rows of profiles/r18_device_math.txt"""
    p = run.probe
    rows = {}

    def measured_bound(name, cap):
        return None if MEASURED[name] is None else U.measured_bound(MEASURED[name], cap)

    w, k, under, bad = U.exp2_errors(run.exp2, i64.x_ref, i64.x, U.exp2_bound(p.exp_deg), i64.x_edge)
    rows["exp2_fast"] = (w, U.exp2_bound(p.exp_deg), f"x = {i64.x[k]!r}; below 2^-1022: {under}", bad)
    w, k, _, bad = U.exp2_errors(run.scaled, i64.uc_ref, i64.uc, U.exp2_bound(p.exp_deg), i64.uc_edge)
    rows["exp2_scaled"] = (w, U.exp2_bound(p.exp_deg), f"u, c = {i64.u[k]!r}, {i64.c[k]!r}", bad)
    for name, out, ref, arg, cap in (("rsqrt", run.rs, i64.rs_ref, i64.r, U.ROOT_CAP), ("sqrt", run.sq, i64.sq_ref, i64.r, U.ROOT_CAP),
                                     ("rcp_nr", run.rcp, i64.q_ref, i64.q, U.RCP_CAP)):
        w, k = U.rel_errors(out, ref)
        rows[name] = (w, measured_bound(name, cap), f"x = {arg[k]!r}")
    w, k = U.angle_errors(run.angle, i64.a_ref)
    rows["angle_abs"] = (w, U.angle_bound(p.asin_deg), f"(y, x) = ({i64.ay[k]!r}, {i64.ax[k]!r}); theta = 0: {run.angle[i64.theta0]!r}")
    w, k = U.angle_errors(run.composed, i64.a_ref.ld[i64.composable])
    root = measured_bound("rsqrt", U.ROOT_CAP)
    rows["angle_abs composed"] = (w, None if root is None else U.angle_bound(p.asin_deg) + U.ROOT_TO_ANGLE * root,
                                  f"(y, x) = ({i64.ay[i64.composable][k]!r}, {i64.ax[i64.composable][k]!r})")
    # f32
    name = "exp2_fast f32"
    w, k, under, bad = U.exp2_errors(run.exp2_f32, i32.x_ref, i32.x, measured_bound(name, U.F32_CAP) or U.F32_CAP, i32.x_edge,
                                 min_normal_exp=-126.0, denormal_ulp=2.0 ** -149)
    rows[name] = (w, measured_bound(name, U.F32_CAP), f"x = {i32.x[k]!r}; below 2^-126: {under}", bad)
    name = "exp2_scaled f32"
    w, k, _, bad = U.exp2_errors(run.scaled_f32, i32.uc_rounded_ref, i32.uc_rounded, measured_bound(name, U.F32_CAP) or U.F32_CAP, i32.uc_edge,
                            min_normal_exp=-126.0, denormal_ulp=2.0 ** -149)
    rows[name] = (w, measured_bound(name, U.F32_CAP), f"u, c = {i32.u[k]!r}, {i32.c[k]!r} (against 2^fl(u c))", bad)
    name = "exp2_scaled f32, exact product, |u c| <= 16"
    near = np.abs(i32.uc) <= F32_SCALED_EXACT_RANGE
    w, k = U.rel_errors(run.scaled_f32[near], i32.uc_ref.ld[near])
    rows[name] = (w, measured_bound(name, U.F32_CAP), f"u, c = {i32.u[near][k]!r}, {i32.c[near][k]!r}")
    for name, out, ref, arg in (("rsqrt f32", run.rs_f32, i32.rs_ref, i32.r), ("sqrt f32", run.sq_f32, i32.sq_ref, i32.r),
                                ("rcp_nr f32", run.rcp_f32, i32.q_ref, i32.q)):
        w, k = U.rel_errors(out, ref)
        rows[name] = (w, measured_bound(name, U.F32_CAP), f"x = {arg[k]!r}")
    w, k = U.angle_errors(run.angle_f32, i32.a_ref)
    rows["angle_abs f32"] = (w, measured_bound("angle_abs f32", U.F32_CAP),
                             f"(y, x) = ({i32.ay[k]!r}, {i32.ax[k]!r}); theta = 0: {run.angle_f32[i32.theta0]!r}")
    return rows


@pytest.fixture(scope="module")
def inputs():
    return Inputs(np.float64), Inputs(np.float32)


@pytest.fixture(scope="module")
def runs(inputs):
    U.make_probe()  # nothing to do when the libraries are up to date; raises with the compiler's output otherwise
    return {b: Run(U.Probe(b), *inputs) for b in BUILDS}


@pytest.fixture(scope="module")
def rows(runs, inputs):
    return {b: figures(runs[b], *inputs) for b in BUILDS}


def test_builds_are_what_they_claim(runs):
    assert (runs["default"].probe.asin_deg, runs["default"].probe.exp_deg, runs["default"].probe.omod) == (7, 9, 1)
    assert (runs["strict"].probe.asin_deg, runs["strict"].probe.exp_deg, runs["strict"].probe.omod) == (8, 9, 1)


F64_ROWS = ["exp2_fast", "exp2_scaled", "rsqrt", "sqrt", "rcp_nr", "angle_abs", "angle_abs composed"]
F32_ROWS = ["exp2_fast f32", "exp2_scaled f32", "exp2_scaled f32, exact product, |u c| <= 16", "rsqrt f32", "sqrt f32", "rcp_nr f32",
            "angle_abs f32"]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", F64_ROWS + F32_ROWS, ids=lambda n: n.replace(" ", "_").replace(",", "").replace("|", ""))
def test_worst_error_within_its_bound(rows, name, build):
    """every function, both builds: the worst error over the whole input set against the bound derived for it (module docstring);
    roots and reciprocal additionally against what "23 good bits" of the seed imply, whatever was measured"""
    worst, bound, where, *bad = rows[build][name]
    print(f"{name} [{build}]: worst error {worst:.3e}, bound {bound:.3e}, at {where}")
    assert not any(bad), bad
    assert worst <= bound
    if name in ("rsqrt", "sqrt"):
        assert worst <= U.ROOT_CAP
    if name == "rcp_nr":
        assert worst <= U.RCP_CAP
    if name in F32_ROWS:
        assert bound <= U.F32_CAP


@pytest.mark.parametrize("build", BUILDS)
def test_exp2_underflow_is_plus_zero(runs, inputs, build):
    """2^-1022 and above are normal results within the bound (test_worst_error_within_its_bound); below, +0 or within the bound
    (exp2_errors, as are no NaN and no negative zero); from 2^-1075 down the only double left is +0"""
    i64, i32 = inputs
    out = runs[build].exp2
    for v in (-1075.0, -1100.0, -1e6, -(1e9 - 1)):
        k = int(np.flatnonzero(i64.x == v)[0])
        assert bits(out[k:k + 1])[0] == 0, (v, out[k])
    deep = i32.x < -150.0
    assert deep.sum() > 1000 and not bits(runs[build].exp2_f32[deep]).any()  # exp2_fast(float) below -150: exactly +0


def test_exp2_is_bit_identical_in_both_builds(runs):
    """both use the degree-9 table"""
    for name in ("exp2", "scaled"):
        assert np.array_equal(bits(getattr(runs["default"], name)), bits(getattr(runs["strict"], name))), name


GATE_OPEN = [1e-300, -1e-300, 1.0, -1.0, 1e300, -1e300, float("nan")]
GATE_DENORMAL = [1e-310, -1e-310]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("build", BUILDS)
def test_gated_pair_of_exponentials(runs, inputs, build, dtype):
    """e1 is exp2_fast(x1) and e2 is exp2_fast(x2), bit for bit — or +0.0, bit for bit, exactly where cw is a zero of either sign.
    A denormal cw is recorded, not required: with FP64 denormals flushed the compare may see a zero."""
    i = inputs[0] if dtype == np.float64 else inputs[1]
    run = runs[build]
    single = run.exp2 if dtype == np.float64 else run.exp2_f32
    n = 8192
    x1 = i.x[:n]
    x2 = i.x[:n][::-1].copy()
    e_x2 = single[:n][::-1]
    for cw in [0.0, -0.0] + GATE_OPEN + GATE_DENORMAL:
        e1, e2 = run.probe.exp2_fast2_gated(x1, x2, np.full(n, cw), dtype=dtype)
        assert np.array_equal(bits(e1), bits(single[:n])), cw
        if cw == 0.0:
            assert not bits(e2).any(), cw
        elif cw in GATE_DENORMAL:
            closed, open_ = not bits(e2).any(), np.array_equal(bits(e2), bits(e_x2))
            print(f"cw = {cw!r} [{build}, {np.dtype(dtype).name}]: the gate is {'closed (e2 = +0)' if closed else 'open (e2 = exp2_fast(x2))'}")
            assert closed or open_, cw
        else:
            assert np.array_equal(bits(e2), bits(e_x2)), cw
    # lanes of one wave with different cw
    cw = np.resize(np.array([0.0, 1.0, -0.0, -1e-300, float("nan")]), n)
    e1, e2 = run.probe.exp2_fast2_gated(x1, x2, cw, dtype=dtype)
    assert np.array_equal(bits(e1), bits(single[:n])) and np.array_equal(bits(e2), np.where(cw == 0.0, np.zeros_like(bits(e_x2)), bits(e_x2)))


@pytest.mark.parametrize("build", BUILDS)
def test_root_identities(runs, inputs, build):
    """sq sq = x and rs sq = 1 to twice the root's bound (+ the rounding of sq = x rs)"""
    i64 = inputs[0]
    run = runs[build]
    bound = 2 * U.measured_bound(MEASURED["sqrt"], U.ROOT_CAP) + 2.0 ** -52
    x, rs, sq = (U.LD(1) * v for v in (i64.r, run.rs, run.sq))
    a, b = float(np.max(np.abs(sq * sq - x) / x)), float(np.max(np.abs(rs * sq - 1)))
    print(f"[{build}] |sq sq - x| / x <= {a:.3e}, |rs sq - 1| <= {b:.3e}, bound {bound:.3e}")
    assert a <= bound and b <= bound


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("build", BUILDS)
def test_angle_range_and_folds(runs, inputs, rows, build, dtype):
    """0 <= theta <= pi everywhere, and across each of the five fold angles (50 points within +-1e-12 of it, f32: +-1e-5, at two
    radii) the result never decreases by more than the bound"""
    f64 = dtype == np.float64
    i = inputs[0] if f64 else inputs[1]
    out = runs[build].angle if f64 else runs[build].angle_f32
    bound = rows[build]["angle_abs" if f64 else "angle_abs f32"][1]
    descent = U.fold_descent(out, i.a_ref, i.folds)
    print(f"[{build}, {np.dtype(dtype).name}] theta = 0 exactly: {out[i.theta0]!r}; min {out.min()!r}, pi - max {np.pi - float(out.max())!r}; "
          f"largest descent across a fold {descent:.3e}, bound {bound:.3e}")
    assert out.min() >= 0 and out.max() <= dtype(np.pi)
    assert descent <= bound
    if f64:
        assert runs[build].composed.min() >= 0 and runs[build].composed.max() <= np.pi


def test_strict_build_angle_is_more_accurate(runs, inputs):
    i64 = inputs[0]
    bulk = slice(i64.a_edge, None)
    err = {b: float(np.max(np.abs(U.LD(1) * runs[b].angle[bulk] - i64.a_ref.ld[bulk]))) for b in BUILDS}
    print(f"angle_abs over the bulk set: default {err['default']:.3e}, strict {err['strict']:.3e}")
    assert err["strict"] < err["default"]


if __name__ == "__main__":  # the table of profiles/r18_device_math.txt
    U.make_probe()
    ins = Inputs(np.float64), Inputs(np.float32)
    print("function | build | worst error | bound | where")
    for b in BUILDS:
        r = Run(U.Probe(b), *ins)
        for name, (worst, bound, where, *_) in figures(r, *ins).items():
            print(f"{name} | {b} | {worst:.3e} | {'(to be measured)' if bound is None else '%.3e' % bound} | {where}")
        for dt, i, single in ((np.float64, ins[0], r.exp2), (np.float32, ins[1], r.exp2_f32)):
            for cw in GATE_DENORMAL:
                _, e2 = r.probe.exp2_fast2_gated(i.x[:64], i.x[:64], np.full(64, cw), dtype=dt)
                print(f"gate, cw = {cw!r} | {b} {np.dtype(dt).name} | {'closed: e2 = +0' if not bits(e2).any() else 'open' if np.array_equal(bits(e2), bits(single[:64])) else 'NEITHER'}")
    sys.exit(0)
