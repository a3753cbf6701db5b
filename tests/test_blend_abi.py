"""Softmin blend (sfw_grid_blend): exported, declared in plain C99, ABI version unchanged, the argument checks that need no
GPU, and the numpy mirror (social_force_window_planner_amd/blend.py) against math.fsum.

The sums of the mirror go through the header's tree: depth d = blend.depth(T) additions at most, one rounded product per
term.  The standard bound for such a sum is |computed - exact| <= gamma_(d+1) * sum |terms| with gamma_m = m u / (1 - m u),
u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); math.fsum of the same terms stands for the
exact sum (it is correctly rounded: within u of it)."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from social_force_window_planner_amd import blend, planner
from social_force_window_planner_amd._abi import (EXPORTED_SYMBOLS, SFW_BLEND_MAX_L, SFW_COST_INVALID, SFW_COST_SKIPPED,
                                                   SFW_ERR_INVALID_ARG, SfwBlendStat)
from sfw_test_util import _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
SIZES = [1, 63, 64, 65, blend.C - 1, blend.C, blend.C + 1, 2 * blend.C + 3, 40000]
LAMBDAS = [0.05, 1.0, 30.0]


def _gamma(m):
    return m * U / (1.0 - m * U)


def test_blend_symbol_declared_and_exported():
    declared = set(re.findall(r"\b(sfw_[a-z_0-9]+)\s*\(", _header()))
    assert "sfw_grid_blend" in declared and "sfw_grid_blend" in EXPORTED_SYMBOLS
    assert hasattr(planner.lib(), "sfw_grid_blend") and planner.exported_symbols()["sfw_grid_blend"]
    assert re.search(r"#define SFW_BLEND_MAX_L 16\b", _header()) and SFW_BLEND_MAX_L == 16 and blend.MAX_L == 16
    assert C.sizeof(SfwBlendStat) == 48
    assert re.search(r"\bC = %d\b" % blend.C, _header())  # the header states the block size the mirror uses


def test_abi_version_unchanged():
    assert planner.lib().sfw_abi_version() == 2
    assert re.search(r"#define SFW_ABI_VERSION 2\b", _header())


def test_header_compiles_as_c99_with_the_blend_call(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "b.c"
    src.write_text('#include "sfw_hip.h"\n#include <stddef.h>\n'
                   "int main(void) { double lam[SFW_BLEND_MAX_L] = {1.0, 0.5}, bias[4] = {0, 0, 0, 0}, u[2 * 3], w[2 * 4];\n"
                   "  sfw_blend_stat st[2];\n"
                   "  return sfw_grid_blend(NULL, lam, 2, bias, st, u, w) + sfw_grid_blend(NULL, lam, 1, NULL, st, u, NULL) +\n"
                   "         (int)(st[0].n_valid + st[0].index_min) + (int)(st[0].lambda + st[0].j_min + st[0].eta + st[0].sum_w2); }\n")
    r = subprocess.run([gcc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_handle_is_invalid_arg_without_gpu():
    L = planner.lib()
    lam = (C.c_double * 2)(1.0, 0.5)
    st = (SfwBlendStat * 2)()
    u = (C.c_double * 6)()
    assert L.sfw_grid_blend(None, C.addressof(lam), 2, None, st, C.addressof(u), None) == SFW_ERR_INVALID_ARG
    assert L.sfw_grid_blend(None, None, 0, None, None, None, None) == SFW_ERR_INVALID_ARG


def test_python_wrapper_checks_before_the_library():
    g = planner.HipScorer._member_view(None, None, object())  # no handle: every check below must come first
    g._mark_staged((7, 1), knots=2)
    for bad in ([0.0], [-1.0], [1.0, float("nan")], [float("inf")], [], [1.0] * (SFW_BLEND_MAX_L + 1)):
        with pytest.raises(ValueError):
            g.blend(bad)
    with pytest.raises(ValueError):
        g.blend([1.0], bias=np.zeros(6))
    with pytest.raises(ValueError):
        g.blend([1.0], bias=np.zeros(8))


def _random_case(T, K, seed):
    rng = np.random.default_rng(seed)
    costs = rng.uniform(0.0, 50.0, T)
    if T > 2:
        bad = rng.random(T) < 0.2
        costs[bad] = np.where(rng.random(int(bad.sum())) < 0.5, SFW_COST_INVALID, SFW_COST_SKIPPED)
        if not np.any(costs >= 0):
            costs[T // 2] = 3.0
        t = int(np.flatnonzero(costs >= 0)[0])  # a tie at the minimum
        costs[t] = costs[int(np.flatnonzero(costs >= 0)[-1])] = costs[costs >= 0].min()
    knots = rng.uniform(-0.7, 0.7, (K, 3, T))
    bias = rng.uniform(-5.0, 5.0, T)
    return costs, knots, bias


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("T", SIZES)
def test_reference_sums_against_fsum(T, K):
    d = blend.depth(T)
    assert d == 6 + 3 + (T + blend.C - 1) // blend.C - 1
    bound = _gamma(d + 1)
    for with_bias in (False, True):
        costs, knots, bias = _random_case(T, K, 1000 * K + T)
        stats, u, w = blend.reference(costs, knots, LAMBDAS, bias if with_bias else None)
        valid = costs >= 0
        J = costs + bias if with_bias else costs
        j_min = J[valid].min()
        assert w.shape == (len(LAMBDAS), T) and u.shape == (len(LAMBDAS), K, 3)
        for l, lam in enumerate(LAMBDAS):
            s = stats[l]
            assert s["lambda"] == lam and s["j_min"] == j_min and s["n_valid"] == int(valid.sum())
            assert s["index_min"] == int(np.flatnonzero(valid & (J == j_min))[-1])
            assert np.all(w[l][~valid] == 0.0) and np.all(w[l][valid & (J == j_min)] == 1.0)
            assert np.array_equal(w[l][valid], np.exp(-((J[valid] - j_min) / lam)))
            wl = w[l].tolist()
            assert abs(s["eta"] - math.fsum(wl)) <= bound * math.fsum(wl)
            sq = (w[l] * w[l]).tolist()
            assert abs(s["sum_w2"] - math.fsum(sq)) <= bound * math.fsum(sq)
            for k in range(K):
                for c in range(3):
                    terms = (w[l] * knots[k, c]).tolist()
                    assert abs(s["eta"] * u[l, k, c] - math.fsum(terms)) <= bound * math.fsum(abs(x) for x in terms), (l, k, c)
        # handing the weights back in reproduces everything bit for bit, and a second call is the first
        stats2, u2, w2 = blend.reference(costs, knots, LAMBDAS, bias if with_bias else None, weights=w)
        assert stats2 == stats and np.array_equal(u2.view(np.uint64), u.view(np.uint64)) and np.array_equal(w2, w)


def test_reference_tree_is_the_documented_one():
    """tree_sum against a scalar restatement of the header's three levels, term by term"""
    rng = np.random.default_rng(7)
    for T in (1, 65, blend.C + 1, 2 * blend.C + 3):
        x = rng.uniform(-1.0, 1.0, T) * 10.0 ** rng.integers(-8, 8, T)
        v = np.zeros(blend.blocks(T) * blend.C)
        v[:T] = x
        total = None
        for b in range(blend.blocks(T)):
            waves = []
            for wv in range(4):
                lanes = [float(q) for q in v[b * blend.C + 64 * wv: b * blend.C + 64 * wv + 64]]
                for dist in (32, 16, 8, 4, 2, 1):
                    lanes = [lanes[i] + lanes[i ^ dist] for i in range(64)]
                assert len(set(lanes)) == 1
                waves.append(lanes[0])
            p = ((waves[0] + waves[1]) + waves[2]) + waves[3]
            total = p if total is None else total + p
        assert float(blend.tree_sum(x)) == total


def test_reference_without_a_valid_sample():
    T, K = 70, 2
    costs = np.where(np.arange(T) % 2 == 0, SFW_COST_INVALID, SFW_COST_SKIPPED)
    knots = np.random.default_rng(3).uniform(-1, 1, (K, 3, T))
    stats, u, w = blend.reference(costs, knots, LAMBDAS, bias=np.ones(T))
    for l, lam in enumerate(LAMBDAS):
        assert stats[l] == {"lambda": lam, "j_min": -1.0, "eta": 0.0, "sum_w2": 0.0, "n_valid": 0, "index_min": -1}
    assert np.all(u == 0.0) and not np.any(np.signbit(u)) and np.all(w == 0.0)


def test_reference_extreme_temperatures():
    costs = np.array([3.0, 1.0, SFW_COST_INVALID, 2.0, 1.0])
    knots = np.arange(15, dtype=np.float64).reshape(1, 3, 5)
    stats, u, w = blend.reference(costs, knots, [1e-300, 1e300])
    assert np.array_equal(w[0], [0.0, 1.0, 0.0, 0.0, 1.0]) and stats[0]["eta"] == 2.0 and stats[0]["index_min"] == 4
    assert np.array_equal(w[1], [1.0, 1.0, 0.0, 1.0, 1.0]) and stats[1]["eta"] == 4.0
    assert np.array_equal(u[0, 0], [(1 + 4) / 2, (6 + 9) / 2, (11 + 14) / 2])
