"""The ensemble's aggregation under a risk (sfw_ensemble_set_risk) restated in numpy: "Risk" in include/sfw_hip.h, step by
step and in its operation order, from the members' captured terms.  Elementwise operations only, so every product, sum and
quotient is rounded on its own as the kernel rounds it; the results are meant to be compared bit for bit.

The visiting order of the tail expectation is a stable argsort of -W along the member axis (descending social work, the lower
member index first among equals).  Members excluded by contact take part as p = 0, W = 0: wherever they land in that order
they take nothing and add +0.0, which changes no bit."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from ._abi import SFW_COST_INVALID, SFW_COST_SKIPPED, SFW_TERM_DISTANCE, SFW_TERM_SOCIAL


def _fma(a, b, c):
    """a * b + c rounded once (the scoring kernels' social term)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def probability_mass(M, probs=None):
    """(p, P): the probabilities an aggregation uses (1.0 / M each without `probs`) and their sum in member order"""
    p = np.full(M, 1.0 / M) if probs is None else np.asarray(probs, dtype=np.float64).reshape(M)
    P = 0.0
    for m in range(M):
        P = P + float(p[m])
    return p, P


def tail_aggregate(W, p, accepting, tail_mass):
    """Step 5 under SFW_ENSEMBLE_MEAN for W[M, T], p[M], accepting[M, T]: (A[T], Pa[T]).  A is NaN where Pa == 0."""
    M, T = W.shape
    pe = np.where(accepting, p[:, None], 0.0)
    We = np.where(accepting, W, 0.0)
    Pa = np.zeros(T)
    for m in range(M):
        Pa = np.where(accepting[m], Pa + p[m], Pa)
    order = np.argsort(-We, axis=0, kind="stable")
    Ws, ps = np.take_along_axis(We, order, axis=0), np.take_along_axis(pe, order, axis=0)
    tau = tail_mass * Pa
    rem, acc = tau.copy(), np.zeros(T)
    for j in range(M):
        take = np.minimum(ps[j], rem)
        acc = acc + take * Ws[j]
        rem = rem - take
    with np.errstate(invalid="ignore", divide="ignore"):
        return acc / tau, Pa


def ensemble_risk(terms, weights, mode, probs=None, tail_mass=1.0, contact_mass=0.0):
    """(costs[T], rejected[T]) of an aggregation under sfw_risk{tail_mass, contact_mass}.

    terms: the members' cost_terms() arrays, (T, 5) each; weights: (vel, distance, angle, costmap, social); mode: "mean" or
    "max"; probs: M probabilities or None."""
    M, T = len(terms), terms[0].shape[0]
    D = np.stack([t[:, SFW_TERM_DISTANCE] for t in terms])
    W = np.stack([t[:, SFW_TERM_SOCIAL] for t in terms])
    p, P = probability_mass(M, probs)
    thr = contact_mass * P
    rejects = D == SFW_COST_INVALID
    skipped = np.any(D == SFW_COST_SKIPPED, axis=0)
    rejected = rejects.sum(axis=0).astype(np.int32)
    R = np.zeros(T)
    for m in range(M):
        R = np.where(rejects[m], R + p[m], R)
    A, Pa = tail_aggregate(W, p, ~rejects, tail_mass)
    invalid = (rejected == M) | ((rejected > 0) if contact_mass == 0.0 else (R > thr)) | (Pa == 0.0)
    if mode == "max":
        A = np.where(rejects, -np.inf, W).max(axis=0)
    elif mode != "mean":
        raise ValueError(f"mode must be 'mean' or 'max', got {mode!r}")
    # the pedestrian-free terms of the lowest-indexed accepting member
    first = np.argmax(~rejects, axis=0)
    t0 = np.stack(terms)[first, np.arange(T)]
    wv, wd, wa, wc, ws = weights
    base = wv * t0[:, 0] + wd * t0[:, 1] + wa * t0[:, 2]
    base = base + wc * t0[:, 3]
    costs = np.full(T, SFW_COST_INVALID)
    for t in np.flatnonzero(~invalid & ~skipped):
        costs[t] = _fma(ws, float(A[t]), float(base[t])) if np.isfinite(A[t]) else A[t]
    costs[skipped] = SFW_COST_SKIPPED
    rejected[skipped] = 0
    return costs, rejected
