"""The polynomial tables of csrc/sfw_math.h on their own terms, without a GPU.

* Every kAsinQ / kExp2P / kAtanPf table is parsed out of the header and its own maximum error measured with mpmath (200 bits,
  4001 points including both ends of the stated interval; tools/gen_poly.py `measure_tables`, which `gen_poly.py check` prints):
  each must stay within 1.05 x the figure written beside it, and equal the values recorded when this test was written.
* A numpy f64 restatement of exp2_fast / exp2_scaled / angle_abs (tests/device_math_util.py: the same operations in the same
  order) is held to the bounds tests/test_device_math_gpu.py holds the device to, on the same inputs: the proof that those
  bounds — derived from the header's figures — are satisfiable in f64 arithmetic.
* Both builds of the probe library cross-compile and export every entry."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import device_math_util as U

# measured when this test was written (tools/gen_poly.py check), three digits
RECORDED = {("kAsinQ", 8): 2.31e-15, ("kAsinQ", 7): 5.39e-14, ("kAsinQ", 6): 1.65e-12,
            ("kExp2P", 9): 1.80e-14, ("kExp2P", 8): 1.05e-12, ("kExp2P", 7): 5.48e-11,
            ("kAtanPf", 4): 1.37e-8, ("kAtanPf as float", 4): 2.84e-8}


@pytest.fixture(scope="module")
def measured():
    return U.gen_poly().measure_tables(points=4001, bits=200)


def test_every_table_of_the_header_is_parsed(measured):
    assert sorted((t["name"], t["degree"]) for t in measured) == sorted(RECORDED)
    assert {t["kind"] for t in measured if t["name"] == "kExp2P"} == {"rel"}
    assert {t["kind"] for t in measured if t["name"] != "kExp2P"} == {"abs"}


@pytest.mark.parametrize("key", sorted(RECORDED), ids=lambda k: f"{k[0].replace(' ', '_')}{k[1]}")
def test_table_error_is_what_its_comment_says(measured, key):
    t = next(t for t in measured if (t["name"], t["degree"]) == key)
    print(f"{key}: measured {t['measured']:.3e} at {t['at']:+.6f}, header {t['stated']:.2e}")
    assert t["measured"] <= 1.05 * t["stated"]
    assert abs(t["measured"] / RECORDED[key] - 1) <= 0.01  # three recorded digits


def test_gen_poly_check_prints_the_measured_errors(measured, capsys):
    assert U.gen_poly().check(measured=measured)
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == len(measured)
    for t, line in zip(measured, lines):
        assert t["name"] in line and "%.3e" % t["measured"] in line and "EXCEEDS" not in line


# ---- the numpy restatement within the device bounds -------------------------------------------------------------------------
def _coef(name, deg):
    return U.tables()[(name, deg)]["coef"]


def test_restated_exp2_fast_within_the_device_bound():
    x, n_edge = U.exp2_inputs()
    ref = U.exp2_reference("2^x", x, np.zeros_like(x), n_edge)
    bound = U.exp2_bound(9)
    worst, i, under, problems = U.exp2_errors(U.np_exp2_fast(_coef("kExp2P", 9), x), ref, x, bound, n_edge)
    print(f"exp2_fast restated: max rel err {worst:.3e} at x = {x[i]!r}, bound {bound:.3e}; underflowing arguments: {under}")
    assert not problems, problems
    assert worst <= bound
    assert under[-1075.0] == "+0" and under[-1e6] == "+0" and under[-(1e9 - 1)] == "+0"


def test_restated_exp2_scaled_within_the_device_bound():
    u, c, n_edge = U.exp2_scaled_inputs()
    hi, lo = U.two_product(u, c)
    ref = U.exp2_reference("2^(u c)", hi, lo, n_edge)
    bound = U.exp2_bound(9)
    worst, i, _, problems = U.exp2_errors(U.np_exp2_scaled(_coef("kExp2P", 9), u, c), ref, hi, bound, n_edge)
    print(f"exp2_scaled restated: max rel err {worst:.3e} at u, c = {u[i]!r}, {c[i]!r}, bound {bound:.3e}")
    assert not problems, problems
    assert worst <= bound


@pytest.mark.parametrize("deg", [7, 8])
def test_restated_angle_abs_within_the_device_bound(deg):
    y, x, n_edge, folds, n_exact = U.angle_inputs()
    ref, rh, _ = U.angle_reference(y, x, n_edge)
    out = U.np_angle_abs(_coef("kAsinQ", deg), y, -x, rh)
    bound = U.angle_bound(deg)
    worst, i = U.angle_errors(out, ref)
    descent = U.fold_descent(out, ref, folds)
    print(f"angle_abs restated, degree {deg}: max abs err {worst:.3e} at (y, x) = ({y[i]!r}, {x[i]!r}), bound {bound:.3e}; "
          f"theta = 0 gives {out[5]!r}; largest descent across a fold {descent:.2e}")
    assert worst <= bound
    assert out.min() >= 0.0 and out.max() <= np.pi
    assert descent <= bound


# ---- the probe library builds ------------------------------------------------------------------------------------------------
def test_both_probe_builds_cross_compile_and_export_every_entry(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc) or shutil.which("make") is None:
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-C", U.CSRC, "mathprobe", f"PROBEDIR={tmp_path}", f"HIPCC={hipcc}"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    for name, degrees in (("libsfw_math_probe.so", (7, 9, 1)), ("libsfw_math_probe_strict.so", (8, 9, 1))):
        lib = ctypes.CDLL(str(tmp_path / name))
        missing = [s for s in U.PROBE_SYMBOLS if not hasattr(lib, s)]
        assert not missing, (name, missing)
        a, e, o = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        lib.probe_config(ctypes.byref(a), ctypes.byref(e), ctypes.byref(o))
        assert (a.value, e.value, o.value) == degrees, name
