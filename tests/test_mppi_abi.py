"""MPPI on the device (sfw_sequences_control_cost, sfw_grid_blend_control, sfw_mppi_run): exported, declared in plain C99, the
struct's size, the argument checks that need no GPU, and the numpy mirror of the control cost
(social_force_window_planner_amd/mppi.py) held against a slow pure-Python loop written from the header's definition: the
summation order, the sigma == 0 skip, gamma == 0, and a 2-knot case worked out by hand."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from social_force_window_planner_amd import mppi, planner
from social_force_window_planner_amd._abi import EXPORTED_SYMBOLS, SFW_ERR_INVALID_ARG, SFW_MPPI_MAX_ITER, SfwMppi
from sfw_test_util import _bits, _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sfw_sequences_control_cost", "sfw_grid_blend_control", "sfw_mppi_run")


def test_symbols_declared_and_exported():
    declared = set(re.findall(r"\b(sfw_[a-z_0-9]+)\s*\(", _header()))
    exported = planner.exported_symbols()
    for s in SYMBOLS:
        assert s in declared and s in EXPORTED_SYMBOLS and hasattr(planner.lib(), s) and exported[s], s
    assert re.search(r"#define SFW_MPPI_MAX_ITER 32\b", _header()) and SFW_MPPI_MAX_ITER == 32
    assert C.sizeof(SfwMppi) == 24
    assert planner.lib().sfw_abi_version() == 2 and re.search(r"#define SFW_ABI_VERSION 2\b", _header())


def test_header_compiles_as_c99_with_the_mppi_calls(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "m.c"
    src.write_text('#include "sfw_hip.h"\n#include <stddef.h>\n'
                   "typedef char size_of_sfw_mppi_is_24[sizeof(sfw_mppi) == 24 ? 1 : -1];\n"
                   "int main(void) { double nominal[2 * 3] = {0.3, 0, 0, 0.3, 0, 0.1}, bias[4], u[2 * 3], plans[3 * 2 * 3], lambda = 0.5;\n"
                   "  int32_t steps[2] = {0, 5};\n"
                   "  sfw_perturb p = {7u, 0, {0.1, 0, 0.2}, {0, 0, -0.5}, {0.7, 0, 0.5}, SFW_PERTURB_NO_VY, 0};\n"
                   "  sfw_mppi m = {3, 0, 0.5, 0.25};\n"
                   "  sfw_robot_state rs = {0, 0, 0, 0, 0, 0};\n"
                   "  sfw_goal_args ga = {1, 1, 1, 2, 0};\n"
                   "  sfw_blend_stat stat[SFW_MPPI_MAX_ITER];\n"
                   "  sfw_best best;\n"
                   "  p.nominal = nominal;\n"
                   "  return sfw_sequences_control_cost(NULL, 0.25, bias) +\n"
                   "         sfw_grid_blend_control(NULL, &lambda, 1, 0.25, NULL, stat, u, NULL) +\n"
                   "         sfw_mppi_run(NULL, &rs, &p, 4, 2, steps, &ga, &m, stat, plans, &best); }\n")
    r = subprocess.run([gcc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_handle_is_invalid_arg_without_gpu():
    L = planner.lib()
    out = (C.c_double * 12)()
    assert L.sfw_sequences_control_cost(None, 0.5, C.addressof(out)) == SFW_ERR_INVALID_ARG
    assert L.sfw_grid_blend_control(None, C.addressof(out), 1, 0.5, None, None, C.addressof(out), None) == SFW_ERR_INVALID_ARG
    assert L.sfw_mppi_run(None, None, None, 4, 1, None, None, None, None, C.addressof(out), None) == SFW_ERR_INVALID_ARG


# ---- the numpy mirror against the header's loop, one Python float operation at a time ------------------------------------------------
def _slow(nominal, sigma, z, gamma):
    K, _, n = z.shape
    out = np.empty(n)
    for t in range(n):
        acc = 0.0
        for k in range(K):
            for c in range(3):
                if sigma[c] > 0.0:
                    q = float(nominal[k][c]) / float(sigma[c])
                    acc = acc + q * float(z[k, c, t])
        out[t] = float(gamma) * acc
    return out


@pytest.mark.parametrize("K,n,sigma", [(1, 1, (0.2, 0.1, 0.3)), (3, 65, (0.2, 0.1, 0.3)), (64, 17, (0.2, 0.0, 0.3)),
                                        (5, 33, (0.0, 0.0, 0.0)), (7, 9, (0.0, 0.3, 0.0))])
def test_control_cost_is_the_loop_of_the_header(K, n, sigma):
    rng = np.random.default_rng(100 * K + n)
    nominal, z = rng.normal(0.2, 0.3, (K, 3)), rng.normal(0.0, 1.0, (K, 3, n))
    got = mppi.control_cost(nominal, sigma, z, 0.37)
    assert got.shape == (n,) and got.dtype == np.float64
    assert np.array_equal(_bits(got), _bits(_slow(nominal, sigma, z, 0.37)))
    if not any(s > 0.0 for s in sigma):
        assert np.all(_bits(got) == 0)


def test_the_order_of_the_sum_is_k_then_c():
    # the same terms in another order round differently: the order is part of the definition
    rng = np.random.default_rng(5)
    nominal, z = rng.normal(0.2, 0.3, (16, 3)), rng.normal(0.0, 1.0, (16, 3, 512))
    sigma = np.array([0.2, 0.1, 0.3])
    got = mppi.control_cost(nominal, sigma, z, 1.0)
    other = np.zeros(512)
    for c in range(3):
        for k in range(16):
            other = other + (nominal[k, c] / sigma[c]) * z[k, c]
    assert np.allclose(got, other, rtol=1e-12, atol=1e-12) and np.any(_bits(got) != _bits(other))
    # ... and q is formed first: (nominal / sigma) * z, not nominal * z / sigma
    late = np.zeros(512)
    for k in range(16):
        for c in range(3):
            late = late + nominal[k, c] * z[k, c] / sigma[c]
    assert np.any(_bits(got) != _bits(late))


def test_zero_sigma_channels_are_skipped_and_gamma_zero_gives_zero():
    rng = np.random.default_rng(6)
    nominal, z = rng.normal(0.2, 0.3, (4, 3)), rng.normal(0.0, 1.0, (4, 3, 40))
    with_vy = mppi.control_cost(nominal, (0.2, 0.1, 0.3), z, 0.5)
    no_vy = mppi.control_cost(nominal, (0.2, 0.0, 0.3), z, 0.5)
    gone = nominal.copy()
    gone[:, 1] = 0.0  # a zero nominal adds q * z = +-0.0: the same sums as the skip
    assert np.any(_bits(with_vy) != _bits(no_vy))
    assert np.array_equal(mppi.control_cost(gone, (0.2, 0.1, 0.3), z, 0.5), no_vy)
    z_nan = z.copy()
    z_nan[:, 1] = np.nan  # a skipped channel is not read
    assert np.array_equal(_bits(mppi.control_cost(nominal, (0.2, 0.0, 0.3), z_nan, 0.5)), _bits(no_vy))
    zero = mppi.control_cost(nominal, (0.2, 0.1, 0.3), z, 0.0)
    assert np.all(zero == 0.0) and np.all((_bits(zero) << np.uint64(1)) == 0)  # +0.0 or -0.0
    assert np.any(np.signbit(zero)) and not np.all(np.signbit(zero))


def test_two_knots_by_hand():
    # q = (0.5 / 0.25, -, -0.75 / 0.5) = (2, -, -1.5) and (1.0 / 0.25, -, 0.25 / 0.5) = (4, -, 0.5); sigma[1] == 0
    nominal = [[0.5, 9.0, -0.75], [1.0, 9.0, 0.25]]
    z = np.array([[[1.0, -2.0], [7.0, 7.0], [2.0, 0.5]], [[0.25, 1.0], [7.0, 7.0], [-4.0, 8.0]]])
    # t = 0: 2 * 1 - 1.5 * 2 + 4 * 0.25 + 0.5 * -4 = 2 - 3 + 1 - 2 = -2;  t = 1: -4 - 0.75 + 4 + 4 = 3.25
    assert mppi.control_cost(nominal, (0.25, 0.0, 0.5), z, 2.0).tolist() == [-4.0, 6.5]
    assert mppi.control_cost(nominal, (0.25, 0.0, 0.5), z, -0.5).tolist() == [1.0, -1.625]


def test_mirror_refuses_bad_shapes_and_values():
    z = np.zeros((2, 3, 4))
    for bad in (lambda: mppi.control_cost(np.zeros((2, 2)), (1, 1, 1), z, 1.0), lambda: mppi.control_cost(np.zeros((3, 3)), (1, 1, 1), z, 1.0),
                lambda: mppi.control_cost(np.zeros((2, 3)), (1, -1, 1), z, 1.0), lambda: mppi.control_cost(np.zeros((2, 3)), (1, 1, 1), z, np.nan),
                lambda: mppi.control_cost(np.full((2, 3), np.inf), (1, 1, 1), z, 1.0)):
        with pytest.raises(ValueError):
            bad()
