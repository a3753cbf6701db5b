"""The softmin blend of include/sfw_hip.h (sfw_grid_blend) restated in numpy: definition and summation tree.

Pure numpy, no GPU.  `reference` forms the weights w_t = exp(-(J_t - J_min) / lambda) and sums eta, sum_w2 and every knot
channel in exactly the tree the header documents, so that with the device's own weights handed in (`weights=`) every output
of the device call is reproduced bit for bit; with `weights=None` the only difference is numpy's exp against the device
library's.  Every product is an elementwise numpy product and every addition an elementwise numpy addition of two float64
arrays (IEEE, one rounding each): no np.sum, no np.dot.

The tree (C = 256 samples per block, 4 waves of 64 lanes, B = ceil(T / C) blocks, terms +0.0 for T <= t < B * C):
  1. wave:   for d = 32, 16, 8, 4, 2, 1 every lane i replaces its value by (its own + lane (i xor d)'s); any lane then
             holds the wave's sum;
  2. block:  ((s_0 + s_1) + s_2) + s_3 over the block's four waves;
  3. blocks: (...((p_0 + p_1) + p_2) ...) + p_(B-1) in block order.
"""
import numpy as np

C = 256      # samples per block
WAVE = 64    # lanes per wave
MAX_L = 16   # SFW_BLEND_MAX_L


def blocks(T):
    return (int(T) + C - 1) // C


def depth(T):
    """d(T): the largest number of additions a term passes through on its way into the sum of T terms."""
    return 6 + (C // WAVE - 1) + (blocks(T) - 1)


def tree_sum(x):
    """The header's summation tree over the last axis of x (float64 [..., T]) -> [...]."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[-1]
    B = max(blocks(T), 1)
    v = np.zeros(x.shape[:-1] + (B * C,), dtype=np.float64)
    v[..., :T] = x
    v = v.reshape(x.shape[:-1] + (B, C // WAVE, WAVE))
    lanes = np.arange(WAVE)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ d]
    s = v[..., 0]                       # [..., B, 4]: every lane holds the wave's sum
    p = s[..., 0]
    for w in range(1, C // WAVE):
        p = p + s[..., w]               # [..., B]
    acc = p[..., 0]
    for b in range(1, B):
        acc = acc + p[..., b]
    return acc


def reference(costs, knots, lambdas, bias=None, weights=None):
    """costs[T]; knots[K, 3, T] = (vx, vy, vtheta) of every knot of every sample (a grid or a list: K = 1; no vy: zeros);
    lambdas[L]; bias[T] or None; weights[L, T] or None (then they replace np.exp, e.g. the device's own).
    Returns (stats, u[L, K, 3], weights[L, T]); stats is a list of L dicts: lambda, j_min, eta, sum_w2, n_valid, index_min."""
    costs = np.ascontiguousarray(np.asarray(costs, dtype=np.float64).reshape(-1))
    T = len(costs)
    knots = np.asarray(knots, dtype=np.float64)
    if knots.ndim != 3 or knots.shape[1] != 3 or knots.shape[2] != T:
        raise ValueError("knots must be a (K, 3, T) array")
    lam = np.asarray(lambdas, dtype=np.float64).reshape(-1)
    L, K = len(lam), knots.shape[0]
    if L < 1 or L > MAX_L or not np.all(np.isfinite(lam)) or not np.all(lam > 0.0):
        raise ValueError("lambdas: 1 .. 16 finite values > 0")
    valid = costs >= 0.0
    n_valid = int(np.count_nonzero(valid))
    J = costs.copy()
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64).reshape(-1)
        if len(b) != T:
            raise ValueError("bias must hold one value per sample")
        J = costs + b
    if n_valid:
        jv = np.where(valid, J, np.inf)
        index_min = int(np.flatnonzero(jv == jv.min())[-1])  # the LARGEST index that holds the minimum
        j_min = float(J[index_min])
    else:
        index_min, j_min = -1, -1.0
    if weights is None:
        w = np.zeros((L, T), dtype=np.float64)
        if n_valid:
            d = J[valid] - j_min
            with np.errstate(over="ignore", under="ignore"):
                for l in range(L):
                    a = d / lam[l]
                    w[l, valid] = np.exp(-a)
    else:
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64)).reshape(L, T)
    with np.errstate(under="ignore"):
        eta = tree_sum(w)                                        # [L]
        sum_w2 = tree_sum(w * w)                                 # [L]
        s = tree_sum(w[:, None, None, :] * knots[None, :, :, :])  # [L, K, 3]
    u = np.zeros((L, K, 3), dtype=np.float64)
    for l in range(L):
        if eta[l] > 0.0:
            u[l] = s[l] / eta[l]
    stats = [{"lambda": float(lam[l]), "j_min": j_min, "eta": float(eta[l]), "sum_w2": float(sum_w2[l]), "n_valid": n_valid,
              "index_min": index_min} for l in range(L)]
    return stats, u, w
