"""Perturbed sequences (sfw_sequences_perturb_stage, sfw_score_perturbed, sfw_sequences_knots, sfw_sequences_normals):
exported, declared in plain C99, ABI version unchanged, the argument checks that need no GPU, and the numpy mirror
(social_force_window_planner_amd/perturb.py): Random123's known answers for Philox4x32-10, the moments of its normals, and
the clamp, SFW_PERTURB_KEEP_NOMINAL, sigma = 0 and SFW_PERTURB_NO_VY as the header states them.

The moment bounds are four standard errors of the sample moment of N independent standard normals: the mean has standard
error 1 / sqrt(N), the variance sqrt(2 / N) and the fourth moment sqrt((E z^8 - (E z^4)^2) / N) = sqrt(96 / N)."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from social_force_window_planner_amd import perturb, planner
from social_force_window_planner_amd._abi import (EXPORTED_SYMBOLS, SFW_ERR_INVALID_ARG, SFW_PERTURB_KEEP_NOMINAL,
                                                   SFW_PERTURB_KEEP_NORMALS, SFW_PERTURB_NO_VY, SFW_SEQ_MAX_KNOTS, SfwPerturb)
from sfw_test_util import _bits, _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sfw_sequences_perturb_stage", "sfw_score_perturbed", "sfw_sequences_knots", "sfw_sequences_normals")


def test_symbols_declared_and_exported():
    declared = set(re.findall(r"\b(sfw_[a-z_0-9]+)\s*\(", _header()))
    exported = planner.exported_symbols()
    for s in SYMBOLS:
        assert s in declared and s in EXPORTED_SYMBOLS and hasattr(planner.lib(), s) and exported[s], s
    h = _header()
    assert re.search(r"#define SFW_PERTURB_KEEP_NOMINAL 1\b", h) and SFW_PERTURB_KEEP_NOMINAL == perturb.KEEP_NOMINAL == 1
    assert re.search(r"#define SFW_PERTURB_NO_VY\s+2\b", h) and SFW_PERTURB_NO_VY == perturb.NO_VY == 2
    assert re.search(r"#define SFW_PERTURB_KEEP_NORMALS 4\b", h) and SFW_PERTURB_KEEP_NORMALS == perturb.KEEP_NORMALS == 4
    assert re.search(r"#define SFW_SEQ_MAX_KNOTS 64\b", h) and SFW_SEQ_MAX_KNOTS == perturb.MAX_KNOTS == 64
    assert C.sizeof(SfwPerturb) == 8 + 8 + 9 * 8 + 8
    assert "6.283185307179586" in h and perturb.TWO_PI == 6.283185307179586


def test_abi_version_unchanged():
    assert planner.lib().sfw_abi_version() == 2
    assert re.search(r"#define SFW_ABI_VERSION 2\b", _header())


def test_header_compiles_as_c99_with_the_perturb_calls(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "p.c"
    src.write_text('#include "sfw_hip.h"\n#include <stddef.h>\n'
                   "int main(void) { double nominal[2 * 3] = {0.3, 0, 0, 0.3, 0, 0.1}, costs[4], out[3][2 * 4], z[2 * 3 * 4];\n"
                   "  int32_t steps[2] = {0, 5};\n"
                   "  sfw_perturb p = {7u, 0, {0.1, 0, 0.2}, {0, 0, -0.5}, {0.7, 0, 0.5},\n"
                   "                   SFW_PERTURB_KEEP_NOMINAL | SFW_PERTURB_NO_VY | SFW_PERTURB_KEEP_NORMALS, 0};\n"
                   "  sfw_robot_state rs = {0, 0, 0, 0, 0, 0};\n"
                   "  sfw_goal_args ga = {1, 1, 1, 2, 0};\n"
                   "  sfw_best best;\n"
                   "  p.nominal = nominal;\n"
                   "  return sfw_sequences_perturb_stage(NULL, &rs, &p, 4, 2, steps, &ga, 0) +\n"
                   "         sfw_score_perturbed(NULL, &rs, &p, 4, 2, steps, &ga, costs, &best) +\n"
                   "         sfw_sequences_knots(NULL, 0, 4, out[0], NULL, out[2]) + sfw_sequences_normals(NULL, 0, 4, z); }\n")
    r = subprocess.run([gcc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_handle_is_invalid_arg_without_gpu():
    L = planner.lib()
    out = (C.c_double * 12)()
    assert L.sfw_sequences_perturb_stage(None, None, None, 4, 1, None, None, 0) == SFW_ERR_INVALID_ARG
    assert L.sfw_score_perturbed(None, None, None, 4, 1, None, None, None, None) == SFW_ERR_INVALID_ARG
    assert L.sfw_sequences_knots(None, 0, 4, C.addressof(out), None, C.addressof(out)) == SFW_ERR_INVALID_ARG
    assert L.sfw_sequences_normals(None, 0, 4, C.addressof(out)) == SFW_ERR_INVALID_ARG


# ---- Philox4x32-10: the known answers of Random123 (kat_vectors) -------------------------------------------------------------------
KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    got = perturb.philox4x32(counter, key)
    assert " ".join("%08x" % int(w) for w in got) == want
    # vectorised: the same block in every element of an array
    got = perturb.philox4x32(tuple(np.full(5, c, dtype=np.uint64) for c in counter), key)
    assert all(" ".join("%08x" % int(w[i]) for w in got) == want for i in range(5))


def test_counter_is_sample_knot_channel():
    """uniforms(seed, n, K, base)[k, c, t] comes from the block at counter (g lo, g hi, k, c) under key (seed lo, seed hi)"""
    seed, base = (0x299f31d0 << 32) | 0xa4093822, (0x85a308d3 << 32) | 0x243f6a88
    u1, u2 = perturb.uniforms(seed, 3, 4, index_base=base - 1)
    w = [int(x) for x in perturb.philox4x32((base & 0xffffffff, base >> 32, 3, 2), (seed & 0xffffffff, seed >> 32))]
    assert u1[3, 2, 1] == ((((w[1] << 32) | w[0]) >> 11) + 1) * 2.0 ** -53
    assert u2[3, 2, 1] == (((w[3] << 32) | w[2]) >> 11) * 2.0 ** -53


def test_uniform_ranges():
    u1, u2 = perturb.uniforms(11, 4096, 2)
    assert np.all(u1 > 0.0) and np.all(u1 <= 1.0) and np.all(u2 >= 0.0) and np.all(u2 < 1.0)
    assert np.all(u1 * 2.0 ** 53 == np.floor(u1 * 2.0 ** 53)) and np.all(u2 * 2.0 ** 53 == np.floor(u2 * 2.0 ** 53))
    assert math.sqrt(106 * math.log(2.0)) < perturb.R_MAX  # u1 >= 2^-53: r = sqrt(-2 log u1) <= sqrt(106 ln 2)


def test_normal_moments():
    z = perturb.normals(seed=3, n=4096, K=4)
    assert z.shape == (4, 3, 4096)
    z = z.reshape(-1)
    N = z.size
    assert N == 49152
    mean, var, m4 = float(z.mean()), float(np.mean(z * z) - z.mean() ** 2), float(np.mean(z ** 4))
    print(f"normals(seed=3): mean {mean * math.sqrt(N):.2f} standard errors, variance {var:.4f}, fourth moment {m4:.3f}")
    assert abs(mean) <= 4.0 / math.sqrt(N)
    assert abs(var - 1.0) <= 4.0 * math.sqrt(2.0 / N)
    assert abs(m4 - 3.0) <= 4.0 * math.sqrt(96.0 / N)
    assert np.max(np.abs(z)) < 8.58


def test_placement_in_the_mirror():
    """a value depends on (seed, g, k, c) alone: shards, prefixes and fewer knots draw the same numbers; seeds differ"""
    z = perturb.normals(5, 130, 6)
    assert np.array_equal(_bits(z[:, :, 65:]), _bits(perturb.normals(5, 65, 6, index_base=65)))
    assert np.array_equal(_bits(z[:, :, :64]), _bits(perturb.normals(5, 64, 6)))
    assert np.array_equal(_bits(z[:3]), _bits(perturb.normals(5, 130, 3)))
    assert not np.array_equal(z, perturb.normals(6, 130, 6))
    # the counter's carry into its second word
    base = 2 ** 32 - 3
    zc = perturb.normals(5, 8, 2, index_base=base)
    for t in range(8):
        assert np.array_equal(_bits(zc[:, :, t:t + 1]), _bits(perturb.normals(5, 1, 2, index_base=base + t)))
    assert len(np.unique(zc)) == zc.size


def test_clamp_nominal_sigma_and_no_vy():
    K, n = 3, 515
    nominal = np.array([[0.3, 0.05, 0.1], [0.4, -0.05, -0.1], [0.2, 0.0, 0.0]])
    sigma, lo, hi = np.array([0.2, 0.1, 0.3]), np.array([0.25, -0.1, -0.2]), np.array([0.45, 0.1, 0.05])
    z = perturb.normals(9, n, K)
    u = perturb.reference(9, nominal, sigma, lo, hi, n)
    assert u.shape == (K, 3, n)
    raw = nominal[:, :, None] + sigma[None, :, None] * z
    assert np.array_equal(_bits(u), _bits(np.clip(raw, lo[None, :, None], hi[None, :, None])))
    cut = (raw < lo[None, :, None]) | (raw > hi[None, :, None])
    assert 0.25 < cut.mean() < 0.75  # the box cuts about half the draws
    assert np.all(u >= lo[None, :, None]) and np.all(u <= hi[None, :, None])
    # the device's own normals handed in replace the mirror's
    z2 = z + 0.125
    assert np.array_equal(_bits(perturb.reference(9, nominal, sigma, lo, hi, n, normals=z2)),
                          _bits(np.clip(nominal[:, :, None] + sigma[None, :, None] * z2, lo[None, :, None], hi[None, :, None])))
    # KEEP_NOMINAL: global sample 0 is the nominal plan (clamped), every other sample is untouched; no sample of a later shard
    wide_lo, wide_hi = np.full(3, -10.0), np.full(3, 10.0)
    free = perturb.reference(9, nominal, sigma, wide_lo, wide_hi, n)
    kept = perturb.reference(9, nominal, sigma, wide_lo, wide_hi, n, flags=perturb.KEEP_NOMINAL)
    assert np.array_equal(_bits(kept[:, :, 0]), _bits(nominal)) and np.array_equal(_bits(kept[:, :, 1:]), _bits(free[:, :, 1:]))
    assert not np.array_equal(free[:, :, 0], nominal)
    assert np.array_equal(_bits(perturb.reference(9, nominal, sigma, wide_lo, wide_hi, 4, index_base=1, flags=perturb.KEEP_NOMINAL)),
                          _bits(free[:, :, 1:5]))
    assert np.array_equal(_bits(perturb.reference(9, nominal, sigma, lo, hi, 1, flags=perturb.KEEP_NOMINAL)[:, :, 0]),
                          _bits(np.clip(nominal, lo, hi)))
    # sigma = 0: every sample is the nominal plan
    still = perturb.reference(9, nominal, np.zeros(3), wide_lo, wide_hi, n)
    assert np.all(still == nominal[:, :, None])
    one = perturb.reference(9, nominal, np.array([0.2, 0.0, 0.3]), wide_lo, wide_hi, n)
    assert np.all(one[:, 1, :] == nominal[:, 1, None]) and np.array_equal(_bits(one[:, 0]), _bits(free[:, 0]))
    # NO_VY: channel 1 is 0.0 whatever the box says; sigma[1] and the nominal vy must be 0
    flat = nominal.copy()
    flat[:, 1] = 0.0
    nv = perturb.reference(9, flat, [0.2, 0.0, 0.3], [-10.0, 0.05, -10.0], [10.0, 0.1, 10.0], n, flags=perturb.NO_VY)
    assert np.all(_bits(nv[:, 1, :]) == 0) and np.array_equal(_bits(nv[:, 0]), _bits(free[:, 0])) and \
        np.array_equal(_bits(nv[:, 2]), _bits(free[:, 2]))
    with pytest.raises(ValueError):
        perturb.reference(9, nominal, [0.2, 0.0, 0.3], wide_lo, wide_hi, n, flags=perturb.NO_VY)
    with pytest.raises(ValueError):
        perturb.reference(9, flat, sigma, wide_lo, wide_hi, n, flags=perturb.NO_VY)


def test_mirror_refuses_what_the_stage_refuses():
    nominal = np.zeros((2, 3))
    ok = ([0.1, 0.1, 0.1], [-1.0] * 3, [1.0] * 3)
    perturb.reference(1, nominal, *ok, 4)
    for bad in (([0.1, -0.1, 0.1], ok[1], ok[2]), (ok[0], [2.0, -1.0, -1.0], ok[2]), ([np.nan, 0.1, 0.1], ok[1], ok[2]),
                (ok[0], [-np.inf, -1.0, -1.0], ok[2]), (ok[0], ok[1], [np.inf, 1.0, 1.0])):
        with pytest.raises(ValueError):
            perturb.reference(1, nominal, *bad, 4)
    with pytest.raises(ValueError):
        perturb.reference(1, np.full((2, 3), np.nan), *ok, 4)
    with pytest.raises(ValueError):
        perturb.normals(1, 0, 2)
    with pytest.raises(ValueError):
        perturb.normals(1, 4, 65)
    with pytest.raises(ValueError):
        perturb.normals(1, 4, 2, index_base=-1)


def test_python_wrapper_shapes():
    g = planner.HipScorer._member_view(None, None, object())  # no handle: the shape checks come before the library
    for bad_nominal, steps in ((np.zeros((2, 2)), (0, 1)), (np.zeros(6), (0, 1)), (np.zeros((2, 3)), (0, 1, 2))):
        with pytest.raises(ValueError):
            g.stage_perturbed((0,) * 6, 4, 1, bad_nominal, [0.1] * 3, [-1.0] * 3, [1.0] * 3, steps, (1, 1, 1, 2, 0))
