"""sfw_ensemble_set_risk / _get_risk (the ensemble's tail expectation and contact-mass bound): declared, exported, callable from
plain C11, refused on a NULL handle, the two kernels built once within the ensemble kernels' budgets, and the properties of the
numpy restatement (social_force_window_planner_amd/risk.py) on synthetic term arrays.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from social_force_window_planner_amd import planner, risk
from social_force_window_planner_amd._abi import (EXPORTED_SYMBOLS, SFW_COST_INVALID, SFW_COST_SKIPPED, SFW_ERR_INVALID_ARG,
                                                   SfwRisk)
from kernel_listing import KERNELS_TU, listing, source
from sfw_test_util import _bits, _header, _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RISK_SYMBOLS = ("sfw_ensemble_set_risk", "sfw_ensemble_get_risk")
# the one translation unit that holds the new kernels (both sit under #ifndef SFW_STRICT_BUILD, as sfw_ens_list_first does)
RISK_TU, RISK_KERNELS = KERNELS_TU, ("sfw_ens_risk_grid", "sfw_ens_risk_list")


def test_risk_symbols_declared_and_exported():
    hdr = _header()
    declared = set(re.findall(r"\b(sfw_[a-z_0-9]+)\s*\(", hdr))
    assert set(RISK_SYMBOLS) <= declared and set(RISK_SYMBOLS) <= set(EXPORTED_SYMBOLS)
    L = planner.lib()
    assert all(hasattr(L, n) for n in RISK_SYMBOLS)
    assert re.search(r"typedef struct sfw_risk \{\s*double tail_mass;[^}]*double contact_mass;[^}]*int64_t reserved;[^}]*\} sfw_risk;", hdr)
    assert C.sizeof(SfwRisk) == 24
    assert "reads `rejected`" not in hdr and "contact_mass" in hdr


def test_risk_header_is_plain_c11(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "r.c"
    src.write_text('#include "sfw_hip.h"\n#include <stddef.h>\n'
                   "int main(void) {\n"
                   "  sfw_ensemble e = NULL; sfw_risk r = {0.25, 0.1, 0}, got; int32_t on = 0;\n"
                   "  int rc = sfw_ensemble_set_risk(e, &r) | sfw_ensemble_set_risk(e, NULL);\n"
                   "  rc |= sfw_ensemble_get_risk(e, &got, &on) | sfw_ensemble_get_risk(e, &got, NULL);\n"
                   "  return rc + on + (got.tail_mass > r.contact_mass) + (int)got.reserved;\n"
                   "}\n")
    r = subprocess.run([gcc, "-std=c11", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_ensemble_is_refused():
    L = planner.lib()
    r, on = SfwRisk(0.5, 0.0, 0), C.c_int32(7)
    assert L.sfw_ensemble_set_risk(None, C.byref(r)) == SFW_ERR_INVALID_ARG
    assert L.sfw_ensemble_set_risk(None, None) == SFW_ERR_INVALID_ARG
    assert L.sfw_ensemble_get_risk(None, C.byref(r), C.byref(on)) == SFW_ERR_INVALID_ARG
    assert (r.tail_mass, r.contact_mass, r.reserved, on.value) == (0.5, 0.0, 0, 7)


@pytest.fixture(scope="module")
def resources():
    return listing(RISK_TU).resources


def test_risk_kernels_within_the_ensemble_budgets(resources):
    res = resources
    for kernel in RISK_KERNELS:
        names = [n for n in res if kernel in n]
        assert len(names) == 1, (kernel, names)
        r = res[names[0]]
        assert r["scratch"] == 0 and r["occupancy"] >= 4 and r["vgpr"] <= 128, (kernel, r)
    # the existing resource tests find kernels by substring: no existing ensemble kernel's name occurs in a new one's
    assert not [n for n in res if "sfw_ens_risk" in n and ("sfw_ensemble_stage" in n or "sfw_ens_list_first" in n)]
    src = source(RISK_TU)
    assert src.index("#ifndef SFW_STRICT_BUILD  // (terms and costs") < src.index("sfw_ens_risk_first(") < \
        src.index("sfw_ens_risk_list(") < src.index("#endif  // SFW_STRICT_BUILD", src.index("sfw_ens_risk_list("))


def test_risk_kernels_use_no_floating_point_atomics():
    src = source(RISK_TU)
    body = src[src.index("sfw_ens_risk_first("):src.index("sfw_ens_risk_list(")]
    assert "atomic" not in body and "#pragma clang fp contract(off)" in body


# ---- the restatement on synthetic terms --------------------------------------------------------------------------------------
WEIGHTS = (0.7, 1.3, 0.4, 2.0, 1.7)


def _terms(W, D=None, seed=0):
    """M members' (T, 5) term arrays: the pedestrian-free terms random and the same in every member, W[m][t] the social work, D
    (optional, [m][t]) the distance term where it is a sentinel — a sentinel sample holds its sentinel in every term"""
    W = np.asarray(W, dtype=np.float64)
    M, T = W.shape
    free = np.random.default_rng(seed).uniform(0.1, 3.0, (T, 4))
    out = []
    for m in range(M):
        t = np.concatenate([free, W[m][:, None]], axis=1)
        if D is not None:
            s = np.asarray(D[m]) < 0
            t[s, :] = np.asarray(D[m], dtype=np.float64)[s, None]
        out.append(t)
    return out


def _base(terms, t=0):
    wv, wd, wa, wc, _ = WEIGHTS
    x = terms[0][t]
    return (wv * x[0] + wd * x[1] + wa * x[2]) + wc * x[3]


def test_worked_example():
    p, W = np.array([0.5, 0.25, 0.25]), np.array([[1.0], [4.0], [2.0]])
    A, Pa = risk.tail_aggregate(W, p, np.ones((3, 1), dtype=bool), 0.5)
    assert Pa[0] == 1.0 and A[0] == 3.0  # (0.25 * 4 + 0.25 * 2) / 0.5
    terms = _terms(W)
    costs, rejected = risk.ensemble_risk(terms, WEIGHTS, "mean", p, tail_mass=0.5)
    assert _same(costs, [risk._fma(WEIGHTS[4], 3.0, _base(terms))]) and rejected.tolist() == [0]


def test_single_member_identity_is_bitwise():
    rng = np.random.default_rng(1)
    T = 64
    W = rng.uniform(0.0, 50.0, (1, T))
    D = np.zeros((1, T))
    D[0, 3], D[0, 7] = SFW_COST_INVALID, SFW_COST_SKIPPED
    terms = _terms(W, D)
    for mode in ("mean", "max"):
        costs, rejected = risk.ensemble_risk(terms, WEIGHTS, mode, [1.0], tail_mass=1.0, contact_mass=0.0)
        want = np.array([risk._fma(WEIGHTS[4], W[0, t], _base(terms, t)) for t in range(T)])
        want[3], want[7] = SFW_COST_INVALID, SFW_COST_SKIPPED
        assert _same(costs, want)
        assert rejected.tolist() == [1 if t == 3 else 0 for t in range(T)]


def _walk(ps, Ws, tau):
    """the walk of step 5 over members already in visiting order, in Python floats"""
    rem, acc = tau, 0.0
    for p, w in zip(ps, Ws):
        take = min(p, rem)
        acc = acc + take * w
        rem = rem - take
    return acc / tau


def test_equal_work_is_visited_in_member_order():
    # members 0 and 1 hold the same W and unequal p, and the tail (0.3 of the mass) ends inside the second one visited: taking
    # member 0 first gives other bits than taking member 1 first
    p, W = [0.1, 0.35, 0.2], np.array([[3.3], [3.3], [1.0]])
    tau = 0.3 * (((0.0 + p[0]) + p[1]) + p[2])
    in_order, swapped = _walk(p, [3.3, 3.3, 1.0], tau), _walk([p[1], p[0], p[2]], [3.3, 3.3, 1.0], tau)
    assert _bits(in_order) != _bits(swapped), "the example does not tell the two orders apart"
    A, _ = risk.tail_aggregate(W, np.array(p), np.ones((3, 1), dtype=bool), 0.3)
    assert _bits(A[0]) == _bits(in_order)
    # unequal W: the larger goes first whatever its index
    A, _ = risk.tail_aggregate(np.array([[3.3], [3.4], [1.0]]), np.array(p), np.ones((3, 1), dtype=bool), 0.3)
    assert _bits(A[0]) == _bits(_walk([p[1], p[0], p[2]], [3.4, 3.3, 1.0], tau))


def _random_case(seed, M=7, T=200):
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.0, 80.0, (M, T))
    W[:, ::5] = np.round(W[:, ::5] / 20.0) * 20.0  # (ties)
    D = np.zeros((M, T))
    D[rng.uniform(size=(M, T)) < 0.15] = SFW_COST_INVALID
    p = rng.uniform(0.0, 1.0, M)
    return W, D, p


def test_cost_does_not_increase_with_the_tail_mass():
    W, D, p = _random_case(2)
    terms = _terms(W, D)
    masses = [0.01, 0.05, 1.0 / 6.0, 0.3, 0.5, 0.75, 1.0]
    costs = [risk.ensemble_risk(terms, WEIGHTS, "mean", p, tail_mass=a, contact_mass=0.6)[0] for a in masses]
    valid = costs[0] >= 0
    assert valid.sum() > 100
    # A CVaR is non-increasing in exact arithmetic.  Rounded it is not, strictly: a tail inside the worst member alone gives
    # (tau * W) / tau, which lands one ulp above or below W depending on tau.  So each of the two costs compared is held to the
    # exact value within the walk's rounding slack, the bound of test_cost_is_at_most_the_worst_case: 2M + 2 rounded operations
    # of at most W_max each, weighted by w_s, and the final fma's rounding.
    slack = (2 * W.shape[0] + 2) * 2.0 ** -53 * WEIGHTS[4] * W.max() + 2.0 ** -52 * np.abs(costs[0][valid])
    for lo, hi in zip(costs[1:], costs[:-1]):
        assert np.array_equal(lo >= 0, valid)
        assert np.all(lo[valid] <= hi[valid] + slack)
    assert np.any(costs[-1][valid] < costs[0][valid])


def test_cost_is_at_most_the_worst_case():
    W, D, p = _random_case(3)
    M = W.shape[0]
    terms = _terms(W, D)
    worst, wr = risk.ensemble_risk(terms, WEIGHTS, "max", p, contact_mass=0.6)
    for a in (0.01, 0.3, 1.0):
        costs, r = risk.ensemble_risk(terms, WEIGHTS, "mean", p, tail_mass=a, contact_mass=0.6)
        valid = costs >= 0
        assert np.array_equal(valid, worst >= 0) and np.array_equal(r, wr) and valid.sum() > 100
        slack = (2 * M + 2) * 2.0 ** -53 * WEIGHTS[4] * W.max() + 2.0 ** -52 * np.abs(costs[valid])
        assert np.all(costs[valid] <= worst[valid] + slack)


def test_zero_probability_member_never_moves_a_result():
    W, D, p = _random_case(4)
    D[0, :] = 0.0  # (member 0 accepts everything: it stays the lowest-indexed accepting member with or without the extra one)
    terms = _terms(W, D)
    rng = np.random.default_rng(5)
    extra_W = rng.uniform(0.0, 200.0, (1, W.shape[1]))
    extra_W[0, ::3] = W[2, ::3]  # (ties with a member that counts)
    with_extra = _terms(np.concatenate([W, extra_W]), np.concatenate([D, np.zeros_like(extra_W)]))
    for a in (0.05, 0.3, 1.0):  # (under "mean": "max" does not read the probabilities)
        for cm in (0.0, 0.4):
            c0, r0 = risk.ensemble_risk(terms, WEIGHTS, "mean", p, tail_mass=a, contact_mass=cm)
            c1, r1 = risk.ensemble_risk(with_extra, WEIGHTS, "mean", np.append(p, 0.0), tail_mass=a, contact_mass=cm)
            assert _same(c0, c1) and np.array_equal(r0, r1), (a, cm)
            assert np.sum(c0 >= 0) > 50


def test_member_excluded_by_contact_is_a_member_absent():
    W, _, p = _random_case(6, M=5)
    T = W.shape[1]
    D = np.zeros_like(W)
    D[3, :] = SFW_COST_INVALID  # member 3 rejects every sample
    full = _terms(W, D)
    keep = [0, 1, 2, 4]
    without = _terms(W[keep], D[keep])
    for mode in ("mean", "max"):
        for a in (0.1, 0.5, 1.0):
            # contact_mass high enough that member 3's share never invalidates a sample
            c_full, r_full = risk.ensemble_risk(full, WEIGHTS, mode, p, tail_mass=a, contact_mass=0.99)
            c_wo, r_wo = risk.ensemble_risk(without, WEIGHTS, mode, p[keep], tail_mass=a, contact_mass=0.99)
            assert np.all(c_full >= 0) and _same(c_full, c_wo), (mode, a)
            assert np.all(r_full == 1) and np.all(r_wo == 0)
    # ... and with contact_mass == 0 it rejects everything, as the plain aggregation does
    c, r = risk.ensemble_risk(full, WEIGHTS, "mean", p, tail_mass=0.5, contact_mass=0.0)
    assert np.all(c == SFW_COST_INVALID) and np.all(r == 1) and len(c) == T


def test_contact_mass_threshold_and_sentinels():
    # M = 4 uniform: one or two rejecting members stay within contact_mass = 0.5 (R = 0.25, 0.5 <= thr = 0.5), three do not
    W = np.array([[1.0] * 6, [2.0] * 6, [3.0] * 6, [4.0] * 6])
    I, S = SFW_COST_INVALID, SFW_COST_SKIPPED
    D = np.array([[0, I, I, I, I, S], [0, 0, I, I, I, S], [0, 0, 0, I, I, S], [0, 0, 0, 0, I, S]], dtype=np.float64)
    terms = _terms(W, D)
    costs, rejected = risk.ensemble_risk(terms, WEIGHTS, "max", None, contact_mass=0.5)
    assert rejected.tolist() == [0, 1, 2, 3, 4, 0]
    assert (costs[:3] >= 0).all() and costs[3] == I and costs[4] == I and costs[5] == S
    # the cost of sample 1 comes from member 1's terms (the lowest-indexed accepting member), MAX over the accepting members
    wv, wd, wa, wc, ws = WEIGHTS
    x = terms[1][1]
    assert _same(costs[1], risk._fma(ws, 4.0, (wv * x[0] + wd * x[1] + wa * x[2]) + wc * x[3]))
    strict, _ = risk.ensemble_risk(terms, WEIGHTS, "max", None, contact_mass=0.0)
    assert (strict >= 0).tolist() == [True, False, False, False, False, False]
    # all accepting probability zero: invalid
    c, _ = risk.ensemble_risk(terms, WEIGHTS, "mean", [1.0, 0.0, 0.0, 0.0], contact_mass=0.999)
    assert c[0] >= 0 and c[1] == I and c[2] == I
