"""What tests/test_device_math_tables.py (CPU) and tests/test_device_math_gpu.py (MI355X) share: the input sets, the
high-precision references (mpmath at the exact inputs for every edge and a random subset, np.longdouble for the bulk, the two
held to 1e-18 of each other), the bounds derived from the figures in csrc/sfw_math.h, a numpy restatement of the f64
functions, and the ctypes binding of the probe library (tests/probe/sfw_math_probe.hip).  No torch."""
import ctypes
import importlib.util
import os
import shutil
import subprocess

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "social_force_window_planner_amd", "csrc")
PROBE_DIR = os.path.join(ROOT, "tests", "probe")
PROBE_LIBS = {"default": os.path.join(PROBE_DIR, "libsfw_math_probe.so"), "strict": os.path.join(PROBE_DIR, "libsfw_math_probe_strict.so")}
LD = np.longdouble
MP_BITS = 200
SEED = 20250318
N_BULK = 100_000   # every call stays under 2^17 elements
N_MP = 3000        # random bulk elements that get an mpmath reference next to all the edges (<= 5000 per function)
SHIFT = 6755399441055744.0  # 1.5 * 2^52
PI = float(np.pi)
ULP_PI = float(np.spacing(np.pi))


def gen_poly():
    spec = importlib.util.spec_from_file_location("sfw_gen_poly", os.path.join(ROOT, "tools", "gen_poly.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_tables = None


def tables():
    """{(name, degree): entry of gen_poly.parse_tables()}"""
    global _tables
    if _tables is None:
        _tables = {(t["name"], t["degree"]): t for t in gen_poly().parse_tables()}
    return _tables


# ---- bounds: from the header's own figures, never from the code under test ---------------------------------------------------
def exp2_bound(exp_deg):
    """1.25 x the table's stated relative error: the margin is the f64 Horner evaluation (10 fma of ~1e-16 each)"""
    return 1.25 * tables()[("kExp2P", exp_deg)]["stated"]


def angle_bound(asin_deg):
    """1.25 x the table's stated absolute error + 4 ulp(pi): the evaluation, the rounding of n (which includes that of rh) and the
    two folds' additions"""
    return 1.25 * tables()[("kAsinQ", asin_deg)]["stated"] + 4 * ULP_PI


ROOT_CAP = 2.2e-14     # "23 good bits" of the seed through one Newton step of rsqrt: 1.5 (2^-23)^2 + rounding
RCP_CAP = 1.5e-14      # ... of the reciprocal: (2^-23)^2 + rounding
F32_CAP = 1e-6         # two decades inside the 1e-4 the f32 mode is held to
ROOT_TO_ANGLE = 0.42   # |n d(asin)/dn| <= tan(pi/8): what a relative error of rh does to the angle


def pow2_ceil(v):
    return float(2.0 ** np.ceil(np.log2(v)))


def measured_bound(measured, cap=None):
    """twice the measured worst error, rounded up to a power of two (room for another input draw), never above `cap`"""
    b = pow2_ceil(2.0 * measured)
    return b if cap is None else min(b, cap)


# ---- references -----------------------------------------------------------------------------------------------------------
def mp_to_ld(v):
    """an mpf as a long double (exact up to the long double's own rounding: mantissa in two doubles, then the exponent)"""
    if v == 0:
        return LD(0)
    m, e = mp.frexp(v)
    hi = float(m)
    lo = float(m - mp.mpf(hi))
    return np.ldexp(LD(hi) + LD(lo), int(max(min(e, 40000), -40000)))


class Reference:
    """`ld`: the long-double reference of every element; `idx`: the elements that have an mpmath value too (every edge, a random
    subset of the bulk).  Construction asserts that the two agree to 1e-18 relative there — where long double is the x87 80-bit
    format; on a machine where it is 64 bits wide this fails instead of letting a weaker reference through — and then takes the
    mpmath values where it has them."""

    def __init__(self, name, ld, idx, mp_values):
        assert np.finfo(LD).eps < 2e-19, "np.longdouble has no 64-bit mantissa here: no reference for the bulk"
        mpv = np.array([mp_to_ld(v) for v in mp_values], dtype=LD)
        ld = np.asarray(ld, dtype=LD).copy()
        dis = np.abs(ld[idx] - mpv)
        bad = dis > LD(1e-18) * np.abs(mpv)
        assert not bad.any(), f"{name}: long double and mpmath disagree at {np.flatnonzero(bad)[:5]}: {ld[idx][bad][:5]} {mpv[bad][:5]}"
        ld[idx] = mpv
        ld.setflags(write=False)
        self.name, self.ld, self.idx = name, ld, idx


def mp_subset(n_edge, n, rng):
    """indices with an mpmath reference: the n_edge leading elements (the edges) and N_MP random ones of the rest"""
    rest = n_edge + rng.choice(n - n_edge, size=min(N_MP, n - n_edge), replace=False)
    return np.concatenate([np.arange(n_edge), np.sort(rest)])


def two_product(a, b):
    """a b = hi + lo exactly (Dekker / Veltkamp, f64; no over- or underflow at the magnitudes used here)"""
    hi = a * b
    def split(v):
        c = 134217729.0 * v
        h = c - (c - v)
        return h, v - h
    ah, al = split(a)
    bh, bl = split(b)
    lo = ((ah * bh - hi) + ah * bl + al * bh) + al * bl
    return hi, lo


# ---- exp2 family ------------------------------------------------------------------------------------------------------------
EXP2_DEEP = [-1021.5, -1022.0, -1022.5, -1074.0, -1075.0, -1100.0, -1e6, -(1e9 - 1)]
TINY_NORMAL = 2.2250738585072014e-308


def exp2_inputs(dtype=np.float64):
    """(x, n_edge): the edges first.  f64: x uniform in [-1000, 10]; every k + 1/2 for k in [-40, 8) with its two neighbours (the
    round-to-even of the shift trick: r = +-1/2); 0, -0.0, +-tiny; the denormal boundary and the argument range's end.
    f32: x uniform in [-160, 10]; the same half-integers; around v_exp_f32's own denormal boundary and the -150 clamp."""
    rng = np.random.default_rng(SEED)
    half = np.arange(-40, 8, dtype=np.float64) + 0.5
    if dtype == np.float64:
        halves = np.concatenate([half, np.nextafter(half, np.inf), np.nextafter(half, -np.inf)])
        edges = np.concatenate([halves, [0.0, -0.0, 5e-324, -5e-324, TINY_NORMAL, -TINY_NORMAL], EXP2_DEEP])
        bulk = rng.uniform(-1000.0, 10.0, N_BULK)
    else:
        h32 = half.astype(np.float32)
        halves = np.concatenate([h32, np.nextafter(h32, np.float32(np.inf)), np.nextafter(h32, np.float32(-np.inf))])
        edges = np.concatenate([halves, np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754944e-38, -1.1754944e-38, -125.5, -126.0, -126.5, -127.0, -148.5,
                                                  -149.0, -149.5, -150.0, -150.5, -151.0, -1100.0, -1e6, -1e9, -3.4e38], dtype=np.float32)])
        bulk = rng.uniform(-160.0, 10.0, N_BULK).astype(np.float32)
    x = np.concatenate([edges, bulk]).astype(dtype)
    return x, len(edges)


def exp2_reference(name, x_hi, x_lo, n_edge):
    """2^(x_hi + x_lo) (x_lo: the exact low part of a product, or 0).  Arguments below -16000 underflow the long double too:
    their reference is 0 there and never used (the true value is below 2^-1022: see exp2_errors)."""
    rng = np.random.default_rng(SEED + 1)
    x_hi = np.asarray(x_hi, dtype=np.float64)
    x_lo = np.asarray(x_lo, dtype=np.float64)
    k = np.rint(np.maximum(x_hi, -16000.0))
    with np.errstate(under="ignore"):
        ld = np.ldexp(np.exp2((LD(1) * np.maximum(x_hi, -16000.0) - k) + x_lo), k.astype(np.int64))
    ld = np.where(x_hi < -16000.0, LD(0), ld)
    idx = mp_subset(n_edge, len(x_hi), rng)
    with mp.workprec(MP_BITS):
        mpv = [mp.power(2, mp.mpf(float(h)) + mp.mpf(float(l))) for h, l in zip(x_hi[idx], x_lo[idx])]
        mpv = [v if h >= -16000.0 else mp.mpf(0) for v, h in zip(mpv, x_hi[idx])]
    return Reference(name, ld, idx, mpv)


def exp2_errors(out, ref, x, bound, n_edge, min_normal_exp=-1022.0, denormal_ulp=None):
    """Relative error of `out` against 2^x where the true value is a normal number; where it lies below 2^min_normal_exp the
    result must be exactly +0 or within the bound (which of the two is returned); never a NaN, never a negative zero.
    `denormal_ulp` (f32 only, where nothing in the project promises a flush): a denormal result passes too when its absolute
    error is within one denormal ulp or within what the bound allows at the smallest normal number, whichever is larger.
    -> (worst relative error over the normal range, its index, {x: '+0' | 'within bound'} of the underflowing x among the n_edge
    leading elements, the violations of the rules above as a list of sentences: empty when all is well)"""
    out = np.asarray(out)
    x = np.asarray(x, dtype=np.float64)
    problems = []
    if np.isnan(out).any():
        problems.append(f"NaN at x = {x[np.isnan(out)][:5]}")
    if (np.signbit(out) & (out == 0)).any():
        problems.append(f"negative zero at x = {x[np.signbit(out) & (out == 0)][:5]}")
    normal = x >= min_normal_exp
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(LD(1) * out.astype(np.float64) - ref.ld)
        rel = np.where(np.isnan(out), np.inf, err / ref.ld)
    worst = int(np.argmax(np.where(normal, rel, 0)))
    under = ~normal
    zero = under & (out == 0)
    close = under & ~zero & (rel <= bound)
    if denormal_ulp is not None:
        close |= under & ~zero & (err <= max(denormal_ulp, bound * 2.0 ** min_normal_exp))
    stray = under & ~zero & ~close
    if stray.any():
        problems.append(f"underflowing arguments {x[stray][:5]} give {out[stray][:5]}: neither +0 nor within {bound:.2e}")
    return (float(rel[worst]), worst, {float(v): ("+0" if z else "within bound") for v, z in zip(x[:n_edge][under[:n_edge]], zero[:n_edge][under[:n_edge]])},
            problems)


def exp2_scaled_inputs(dtype=np.float64):
    """(u, c, n_edge): u log-uniform in [1e-3, 1e3], c uniform in [-50, -0.1]; in front, products that land exactly on half-integers
    (u = 2^j (2 m + 1), c = -2^-(j + 1)) and on integers.  f32: u c in [-140, 0]."""
    rng = np.random.default_rng(SEED + 2)
    m = np.arange(0, 40, dtype=np.float64)
    u_e = np.concatenate([4.0 * (2 * m + 1), 0.25 * (2 * m + 1), 3.0 * (m + 1)])
    c_e = np.concatenate([np.full(40, -0.125), np.full(40, -2.0), np.full(40, -1.0 / 3.0)])
    if dtype == np.float64:
        u = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), N_BULK))
        c = rng.uniform(-50.0, -0.1, N_BULK)
    else:
        u = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), N_BULK))
        c = rng.uniform(-50.0, -0.1, N_BULK)
        c = np.where(u * c < -140.0, -140.0 / u * rng.uniform(0.0, 1.0, N_BULK), c)
    return np.concatenate([u_e, u]).astype(dtype), np.concatenate([c_e, c]).astype(dtype), len(u_e)


# ---- roots and reciprocal ---------------------------------------------------------------------------------------------------
def root_inputs(dtype=np.float64):
    """(x, n_edge).  f64: 10^U(-300, 300); the callers' clamps (1e-300, and tiny + d^2 for d^2 = 0, 1e-290, 1e-16); exact powers of
    4; 1; 2^1022, the largest x whose seed y = 2^-511 still has a normal square (above it y y is flushed and the Newton step is
    void: outside the function's domain).  f32: 10^U(-30, 30), tiny = 1e-30."""
    rng = np.random.default_rng(SEED + 3)
    if dtype == np.float64:
        tiny = 1e-300
        edges = np.concatenate([[tiny, tiny + 0.0, tiny + 1e-290, tiny + 1e-16, 1.0, 2.0 ** 1022, np.nextafter(2.0 ** 1022, 0)],
                                4.0 ** np.arange(-498, 511, 21, dtype=np.float64)])
        bulk = 10.0 ** rng.uniform(-300, 300, N_BULK)
    else:
        tiny = np.float32(1e-30)
        edges = np.concatenate([np.array([tiny, tiny + np.float32(1e-25), tiny + np.float32(1e-16), 1.0], dtype=np.float32),
                                (4.0 ** np.arange(-60, 61, 5, dtype=np.float64)).astype(np.float32)])
        bulk = (10.0 ** rng.uniform(-30, 30, N_BULK)).astype(np.float32)
    return np.concatenate([edges, bulk]).astype(dtype), len(edges)


def root_references(x, n_edge):
    """(1 / sqrt(x), sqrt(x))"""
    rng = np.random.default_rng(SEED + 4)
    idx = mp_subset(n_edge, len(x), rng)
    sq = np.sqrt(LD(1) * x.astype(np.float64))
    with mp.workprec(MP_BITS):
        mps = [mp.sqrt(mp.mpf(float(v))) for v in x[idx]]
        return Reference("1/sqrt", LD(1) / sq, idx, [1 / v for v in mps]), Reference("sqrt", sq, idx, mps)


def rcp_inputs(dtype=np.float64):
    """(x, n_edge): +-10^U(-300, 300) (f32: +-30); the integers 1 .. 100 (the callers divide by counts) and powers of two"""
    rng = np.random.default_rng(SEED + 5)
    span = 300 if dtype == np.float64 else 30
    edges = np.concatenate([np.arange(1.0, 101.0), 2.0 ** np.arange(-span // 2, span // 2, 7, dtype=np.float64)])
    bulk = 10.0 ** rng.uniform(-span, span, N_BULK) * rng.choice([-1.0, 1.0], N_BULK)
    return np.concatenate([edges, bulk]).astype(dtype), len(edges)


def rcp_reference(x, n_edge):
    rng = np.random.default_rng(SEED + 6)
    idx = mp_subset(n_edge, len(x), rng)
    with mp.workprec(MP_BITS):
        return Reference("1/x", LD(1) / (LD(1) * x.astype(np.float64)), idx, [1 / mp.mpf(float(v)) for v in x[idx]])


def rel_errors(out, ref):
    """(worst relative error, its index); `ref`: a Reference or its long-double array"""
    ld = getattr(ref, "ld", ref)
    rel = np.abs(LD(1) * np.asarray(out).astype(np.float64) - ld) / np.abs(ld)
    rel = np.where(np.isnan(rel), np.inf, rel)  # a NaN result is an infinite error
    i = int(np.argmax(rel))
    return float(rel[i]), i


# ---- angle ------------------------------------------------------------------------------------------------------------------
FOLDS = [0.0, PI / 4, PI / 2, 3 * PI / 4, PI]
EDGE_RADII = [1e-150, 1e-3, 0.5, 1.0, 3.0, 1e3, 1e150]
FOLD_RADII = [1.0, 7.3]
N_FOLD = 50


def angle_inputs(dtype=np.float64):
    """(y, x, n_edge, fold_slices, n_exact): the n_exact exact configurations (y, x) in {(0, r), (r, r), (r, 0), (r, -r), (0, -r)} for every r of
    EDGE_RADII (f32: without 1e+-150); 50 points within +-1e-12 (f32: +-1e-5) of each fold angle per radius of FOLD_RADII (the
    outer halves at 0 and pi are mirrored into y >= 0); then theta uniform in [0, pi] x radius 10^U(-3, 3).
    fold_slices: one slice per (fold, radius), for the monotonicity check."""
    rng = np.random.default_rng(SEED + 7)
    ys, xs = [], []
    for r in EDGE_RADII:
        if dtype == np.float32 and not 1e-30 < r < 1e30:
            continue
        ys += [0.0, r, r, r, 0.0]
        xs += [r, r, 0.0, -r, -r]
    n_exact = len(ys)
    width = 1e-12 if dtype == np.float64 else 1e-5
    slices = []
    for f in FOLDS:
        for r in FOLD_RADII:
            th = f + np.linspace(-width, width, N_FOLD)
            slices.append(slice(len(ys), len(ys) + N_FOLD))
            ys += list(np.abs(r * np.sin(th)))
            xs += list(r * np.cos(th))
    n_edge = len(ys)
    th = rng.uniform(0.0, PI, N_BULK)
    rad = 10.0 ** rng.uniform(-3, 3, N_BULK)
    y = np.concatenate([ys, np.abs(rad * np.sin(th))]).astype(dtype)
    x = np.concatenate([xs, rad * np.cos(th)]).astype(dtype)
    return y, x, n_edge, slices, n_exact


def angle_reference(y, x, n_edge):
    """|atan2(y, x)| at the exact inputs, and rh = 1 / hypot(x, y), hyp = hypot(x, y) correctly rounded to the inputs' type"""
    rng = np.random.default_rng(SEED + 8)
    idx = mp_subset(n_edge, len(y), rng)
    yl, xl = LD(1) * y.astype(np.float64), LD(1) * x.astype(np.float64)
    with mp.workprec(MP_BITS):
        ref = Reference("atan2", np.arctan2(yl, xl), idx, [mp.atan2(mp.mpf(float(a)), mp.mpf(float(b))) for a, b in zip(y[idx], x[idx])])
    hyp = np.sqrt(xl * xl + yl * yl)
    return ref, (LD(1) / hyp).astype(y.dtype), hyp.astype(y.dtype)


def angle_errors(out, ref):
    """(worst absolute error, its index); `ref`: a Reference or its long-double array"""
    out = np.asarray(out).astype(np.float64)
    err = np.abs(LD(1) * out - getattr(ref, "ld", ref))
    err = np.where(np.isnan(err), np.inf, err)  # a NaN result is an infinite error
    i = int(np.argmax(err))
    return float(err[i]), i


def fold_descent(out, ref, slices):
    """the largest amount by which the result DEcreases between two points of one fold's neighbourhood, ordered by true angle"""
    worst = 0.0
    for s in slices:
        o = np.asarray(out[s]).astype(np.float64)[np.argsort(ref.ld[s], kind="stable")]
        worst = max(worst, float(np.max(np.maximum.accumulate(o) - o)))
    return worst


# ---- numpy f64 restatement of the device functions: the same operations in the same order, plain multiply-add where the device
# has an fma (except exp2_scaled's two, whose single rounding of u c is the point of the function: exact through two_product);
# results and inputs below the smallest normal are flushed as the kernels' FP mode does ----------------------------------------------
def _flush(v):
    return np.where(np.abs(v) < TINY_NORMAL, 0.0, v)


def _exp2_poly(P, r):
    p = np.full_like(r, P[-1])
    for a in P[-2::-1]:
        p = p * r + a
    return p


def _ldexp_flushed(p, t):
    k = (t - SHIFT).astype(np.int64)  # the device reads the low dword of t: the same integer for |k| < 2^31
    with np.errstate(under="ignore"):
        return _flush(np.ldexp(p, np.maximum(k, -5000)))


def np_exp2_fast(P, x):
    x = _flush(np.asarray(x, dtype=np.float64))
    t = x + SHIFT
    k = t - SHIFT
    return _ldexp_flushed(_exp2_poly(P, x - k), t)


def np_exp2_scaled(P, u, c):
    hi, lo = two_product(np.asarray(u, dtype=np.float64), np.asarray(c, dtype=np.float64))
    t = hi + SHIFT  # fma(u, c, shift): differs from this only where hi is a half-integer and lo != 0 — r is then -+1/2 either way
    k = t - SHIFT
    return _ldexp_flushed(_exp2_poly(P, (hi - k) + lo), t)  # hi - k is exact: one rounding, as fma(u, c, -k)


def np_angle_abs(Q, y, nx, rh):
    y, nx, rh = (np.asarray(v, dtype=np.float64) for v in (y, nx, rh))
    ax = np.abs(nx)
    d, p = y - ax, y + ax
    nu = p * 2.70598050073098492e-01 - np.abs(d) * 6.53281482438188264e-01
    n = nu * rh
    z = n * n
    q = np.full_like(z, Q[-1])
    for a in Q[-2::-1]:
        q = q * z + a
    e = n * q + -3.92699081698724155e-01
    f = np.copysign(e, d) - 7.85398163397448310e-01
    return np.copysign(f, nx) + 1.57079632679489661923


# ---- the probe library ----------------------------------------------------------------------------------------------------
PROBE_ENTRIES = {  # name: (inputs, outputs)
    "rsqrt_sqrt": (1, 2), "rcp_nr": (1, 1), "exp2_fast": (1, 1), "exp2_scaled": (2, 1), "exp2_fast2_gated": (3, 2), "angle_abs": (4, 1)}
PROBE_SYMBOLS = ["probe_config", "probe_angle_abs_composed_f64"] + [f"probe_{n}_{t}" for n in PROBE_ENTRIES for t in ("f64", "f32")]


def make_probe():
    """`make -C csrc mathprobe`: nothing to do when both libraries are newer than their sources; raises with the compiler's output
    when one is missing and cannot be built"""
    if shutil.which("make") is None or (shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc")):
        missing = [p for p in PROBE_LIBS.values() if not os.path.exists(p)]
        if missing:
            raise RuntimeError(f"no make / hipcc to build {missing}")
        return
    env = dict(os.environ)
    if shutil.which("hipcc") is None:
        env["HIPCC"] = "/opt/rocm/bin/hipcc"
    r = subprocess.run(["make", "-C", CSRC, "mathprobe"], capture_output=True, text=True, env=env, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("make mathprobe failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])


class Probe:
    """One build of the probe library.  Every method takes numpy arrays and returns the outputs as new arrays; a hipError_t
    other than hipSuccess raises."""

    def __init__(self, build):
        self.build = build
        self.lib = ctypes.CDLL(PROBE_LIBS[build])
        a, e, o = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self.lib.probe_config(ctypes.byref(a), ctypes.byref(e), ctypes.byref(o))
        self.asin_deg, self.exp_deg, self.omod = a.value, e.value, o.value

    def _call(self, symbol, dtype, inputs, n_out, cw=None):
        n = len(inputs[0])
        assert 0 < n <= 1 << 17 and all(len(v) == n for v in inputs)
        ins = [np.ascontiguousarray(v, dtype=dtype) for v in inputs]
        if cw is not None:
            ins.append(np.ascontiguousarray(cw, dtype=np.float64))
        outs = [np.full(n, np.nan, dtype=dtype) for _ in range(n_out)]
        fn = getattr(self.lib, symbol)
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p] * (len(ins) + n_out) + [ctypes.c_int]
        rc = fn(*[v.ctypes.data for v in ins + outs], n)
        if rc != 0:
            raise RuntimeError(f"{symbol}: hipError_t {rc}")
        return outs[0] if n_out == 1 else tuple(outs)

    @staticmethod
    def _suffix(dtype):
        return {np.float64: "f64", np.float32: "f32"}[dtype]

    def rsqrt_sqrt(self, x, dtype=np.float64):
        return self._call(f"probe_rsqrt_sqrt_{self._suffix(dtype)}", dtype, [x], 2)

    def rcp_nr(self, x, dtype=np.float64):
        return self._call(f"probe_rcp_nr_{self._suffix(dtype)}", dtype, [x], 1)

    def exp2_fast(self, x, dtype=np.float64):
        return self._call(f"probe_exp2_fast_{self._suffix(dtype)}", dtype, [x], 1)

    def exp2_scaled(self, u, c, dtype=np.float64):
        return self._call(f"probe_exp2_scaled_{self._suffix(dtype)}", dtype, [u, c], 1)

    def exp2_fast2_gated(self, x1, x2, cw, dtype=np.float64):
        return self._call(f"probe_exp2_fast2_gated_{self._suffix(dtype)}", dtype, [x1, x2], 2, cw=cw)

    def angle_abs(self, y, nx, rh, hyp, dtype=np.float64):
        return self._call(f"probe_angle_abs_{self._suffix(dtype)}", dtype, [y, nx, rh, hyp], 1)

    def angle_abs_composed(self, y, nx):
        return self._call("probe_angle_abs_composed_f64", np.float64, [y, nx], 1)
