#!/usr/bin/env python3
"""The polynomial tables of the device math in social_force_window_planner_amd/csrc/sfw_math.h.

    python tools/gen_poly.py check      measure every table of the header against mpmath (what the comments beside them claim)
    python tools/gen_poly.py legacy     print the half-angle atan / base-e exp sets of round 1 and the float atan set

What is true about the tables' origin: `legacy` is the generator of round 1.  Its float set (degree 4 in t^2) is the kAtanPf
the f32 mode still uses; its double sets (kAtanP, kExpP) are no longer used by any kernel.  The tables the f64 kernels use
since round 3 — kAsinQ (asin(n) = n Q(n^2) on |n| <= sin(pi/8), degrees 6 / 7 / 8) and kExp2P (2^r on |r| <= 1/2, degrees
7 / 8 / 9) — are not produced by `legacy` or by any other program here: their generator is NOT in the tree.  `check` does not
need it: it parses the literals out of the header and measures each polynomial's own error (coefficients as the doubles the
compiler reads, evaluation and reference in mpmath at 200 bits), which is what tests/test_device_math_tables.py holds to the
figure written beside each table.  The float table is measured twice: as written (the decimal literals, what `legacy`
reports) and with every coefficient rounded to float as the compiler does — the leading 1.999999963 becomes 2.0f, which
doubles the error at the upper end of the interval."""
import os
import re
import sys

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "social_force_window_planner_amd", "csrc",
                      "sfw_math.h")

_F64_TABLE = re.compile(r"#(?:el)?if SFW_(ASIN|EXP)_DEG == (\d+)\s*//\s*max (abs|rel) err ([0-9.]+e[-+]?\d+)\s*\n"
                        r"__device__ constexpr double (kAsinQ|kExp2P)\[(\d+)\] = \{([^}]*)\};")
_F32_TABLE = re.compile(r"//[^\n]*max (abs) err ([0-9.]+e[-+]?\d+) as written, ([0-9.]+e[-+]?\d+) as float[^\n]*\n(?://[^\n]*\n)*"
                        r"__device__ constexpr float (kAtanPf)\[(\d+)\] = \{([^}]*)\};")


def parse_tables(header=HEADER):
    """[{name, degree, kind ('abs' | 'rel'), stated, coef}] — every kAsinQ / kExp2P / kAtanPf table of the header, `coef` as
    correctly rounded doubles of the literals, `stated` the error figure of the table's own comment.  kAtanPf appears twice:
    as written, and ("kAtanPf as float") with the coefficients rounded to float and the comment's second figure."""
    text = open(header).read()
    out = []
    for m in _F64_TABLE.finditer(text):
        which, deg, kind, stated, name, size, body = m.groups()
        coef = [float(v) for v in body.replace("\n", " ").split(",")]
        assert (which, name) in (("ASIN", "kAsinQ"), ("EXP", "kExp2P")) and len(coef) == int(size) == int(deg) + 1, m.group(0)
        out.append(dict(name=name, degree=int(deg), kind=kind, stated=float(stated), coef=coef))
    for m in _F32_TABLE.finditer(text):
        kind, stated, stated_f32, name, size, body = m.groups()
        coef = [float(v.strip().rstrip("f")) for v in body.split(",")]
        assert len(coef) == int(size), m.group(0)
        out.append(dict(name=name, degree=int(size) - 1, kind=kind, stated=float(stated), coef=coef))
        out.append(dict(name=name + " as float", degree=int(size) - 1, kind=kind, stated=float(stated_f32),
                        coef=[float(np.float32(v)) for v in coef]))
    return out


def measure_tables(header=HEADER, points=4001, bits=200):
    """parse_tables() plus, per table, `measured` (the polynomial's own maximum error on its stated interval, over `points`
    equidistant arguments including both ends) and `at` (the argument of the maximum):
      kAsinQ   n Q(n^2) against asin(n) on |n| <= sin(pi/8), absolute;
      kExp2P   P(r) against 2^r on |r| <= 1/2, relative;
      kAtanPf  t P(t^2) against 2 atan(t) on [0, tan(pi/8)], absolute."""
    import mpmath as mp

    tables = parse_tables(header)
    with mp.workprec(bits):
        def horner(c, z):
            p = mp.mpf(c[-1])
            for a in c[-2::-1]:
                p = p * z + mp.mpf(a)
            return p

        cases = {"kAsinQ": (-mp.sin(mp.pi / 8), mp.sin(mp.pi / 8), lambda c, n: abs(n * horner(c, n * n) - mp.asin(n))),
                 "kExp2P": (mp.mpf(-0.5), mp.mpf(0.5), lambda c, r: abs(horner(c, r) / mp.power(2, r) - 1)),
                 "kAtanPf": (mp.mpf(0), mp.tan(mp.pi / 8), lambda c, t: abs(t * horner(c, t * t) - 2 * mp.atan(t)))}
        for t in tables:
            lo, hi, err = cases[t["name"].split()[0]]
            worst, at = mp.mpf(-1), None
            for i in range(points):
                x = lo + (hi - lo) * i / (points - 1)
                e = err(t["coef"], x)
                if e > worst:
                    worst, at = e, x
            t["measured"], t["at"] = float(worst), float(at)
    return tables


def check(header=HEADER, measured=None):
    """prints one line per table (`measured`: the result of measure_tables(), where the caller has it already); False where a
    table exceeds 1.05 x the figure of its comment"""
    ok = True
    for t in measured if measured is not None else measure_tables(header):
        within = t["measured"] <= 1.05 * t["stated"]
        ok &= within
        print("%-16s degree %d: max %s err %.3e at %+.6f (header: %.2e)%s" % (t["name"], t["degree"], t["kind"], t["measured"], t["at"],
                                                                             t["stated"], "" if within else "  EXCEEDS 1.05 x"))
    return ok


# ---- round 1's generator -------------------------------------------------------------------------------------------------
def fit(fn, lo, hi, deg):
    from numpy.polynomial import Chebyshev, Polynomial

    ch = Chebyshev.interpolate(fn, deg, domain=[lo, hi])
    return ch.convert(kind=Polynomial, domain=[-1, 1], window=[-1, 1]).coef


def horner(c, x):
    y = np.full_like(x, c[-1])
    for a in c[-2::-1]:
        y = y * x + a
    return y


def legacy():
    """Near-minimax (Chebyshev interpolation), converted to the monomial basis and verified with a float64 Horner evaluation."""
    # half-angle form: phi in [0, pi/4] is evaluated as phi = t * P(t*t) with
    # t = tan(phi/2) = min/(max + hypot) in [0, tan(pi/8)]  (P includes the factor 2)
    tmax = np.tan(np.pi / 8)

    def g(z):
        t = np.sqrt(np.maximum(z, 0.0))
        return np.where(t > 1e-8, 2 * np.arctan(t) / np.where(t > 0, t, 1.0), 2.0 - 2 * z / 3.0)

    ca = fit(g, 0.0, tmax * tmax * 1.0001, 8)
    q = np.linspace(0, tmax, 400001)
    err = np.abs(q * horner(ca, q * q) - 2 * np.arctan(q))
    print("// 2*atan(t) = t * P(t*t), t in [0, tan(pi/8)]; max abs err %.2e (float64 Horner)" % err.max())
    print("constexpr double kAtanP[%d] = {" % len(ca))
    print(",\n".join("    %.17e" % v for v in ca) + "};")
    h = np.log(2.0) / 2
    ce = fit(np.exp, -h * 1.0001, h * 1.0001, 9)
    r = np.linspace(-h, h, 400001)
    err = np.abs(horner(ce, r) / np.exp(r) - 1)
    print("// exp(r), |r| <= ln2/2; max rel err %.2e" % err.max())
    print("constexpr double kExpP[%d] = {" % len(ce))
    print(",\n".join("    %.17e" % v for v in ce) + "};")
    # float version (f32 mode): atan of degree 4 in z = t*t; 2^x is v_exp_f32
    ca32 = fit(g, 0.0, tmax * tmax * 1.0001, 4)
    err = np.abs(q * horner(ca32, q * q) - 2 * np.arctan(q))
    print("// float atan: max abs err %.2e" % err.max())
    print("constexpr float kAtanPf[%d] = {" % len(ca32))
    print(",\n".join("    %.9ef" % v for v in ca32) + "};")


if __name__ == "__main__":
    if sys.argv[1:] == ["check"]:
        sys.exit(0 if check() else 1)
    if sys.argv[1:] == ["legacy"]:
        legacy()
        sys.exit(0)
    sys.exit(__doc__)
