"""The exact layer of the path term (include/sfw_hip.h "the path term"): D and p in rational arithmetic, and the forward-error
bound a float64 evaluation of the header's expressions is held to.  A plain module: nothing pytest collects.

WHAT IS EXACT.  The contract defines D on the segment RECORDS {ax, ay, ex, ey, inv} — doubles the host forms — so the exact
layer takes a record's five doubles and a pose's two as rationals (every double is one) and evaluates
    rx = px - ax;  ry = py - ay;  u = (rx ex + ry ey) inv;  t = clamp(u, 0, 1);  q = r - t e;  d = qx^2 + qy^2
without any rounding (fractions.Fraction).  D = min d, p = (sum D_i) / S, exact as well.

THE BOUND, from the rounding count.  eps = 2^-53 (round to nearest, no underflow: every non-zero magnitude here is far above
2^-1022; no overflow: |coordinate| <= 1e7).  g(k) = (1 + eps)^k - 1.  R = |r|, E = |e| (2-norms of the EXACT r and of the
record's e), c = E^2 inv (1 for an ideal record, within a few eps of 1 for a real one, 0 for a zero-length segment).
  1. rx~ = rx (1 + d1): one rounding each for rx, ry.
  2. u~: each of the two products carries rx's rounding, its own, the sum's and the final product's: four roundings, so
         |u~ - u| <= g(4) (|rx ex| + |ry ey|) inv <= g(4) R E inv                  (Cauchy-Schwarz)
  3. the clamp is 1-Lipschitz and exact: |t~ - t| <= |u~ - u|, and 0 <= t~ <= 1.
  4. qx~ = (rx~ - t~ ex (1 + d2)) (1 + d3).  Against qx = rx - t ex:
         |qx~ - qx| <= eps |rx| + (|t~ - t| + eps) |ex| + eps (1 + eps) (|rx| + |ex|)
     and in 2-norm, with a = 2 eps + eps^2:
         |q~ - q| <= a (R + E) + |u~ - u| E <= a (R + E) + g(4) c R <= b (R + E),      b = a + g(4) c
  5. d~ = (qx~^2 (1 + d4) + qy~^2 (1 + d5)) (1 + d6): |d~ - |q~|^2| <= g(2) |q~|^2, and ||q~|^2 - |q|^2| <= 2 |q| |q~ - q| + |q~ - q|^2
     with |q| <= R + E (0 <= t <= 1).  Together
         |d~ - d| <= (R + E)^2 [ g(2) (1 + b)^2 + 2 b + b^2 ] <= 2 (R^2 + E^2) [ g(2) (1 + b)^2 + 2 b + b^2 ]
     which is about 28 eps (|r|^2 + |e|^2) for c = 1.
  6. D~ = min_k d~_k (a minimum is exact): |D~ - D| <= max_k bound_k.
  7. p~ = (sum_i D~_i (1 + th_i)) (1 + d) / S with |th_i| <= g(S - 1) (the sum starts from 0.0, whose first addition is exact),
     then the division's rounding:
         |p~ - p| <= (sum_i |D~_i - D_i|) / S + g(S) (sum_i (D_i + |D~_i - D_i|)) / S
Everything in the bound is evaluated in rationals too; nothing is fitted to what path.py returns."""
from fractions import Fraction as F

import numpy as np

EPS = F(1, 2 ** 53)


def g(k):
    return (1 + EPS) ** k - 1


def exact_d(px, py, rec):
    """(d, bound) of one pose against one record, both Fractions"""
    px, py = F(float(px)), F(float(py))
    ax, ay, ex, ey, inv = (F(float(v)) for v in rec)
    rx, ry = px - ax, py - ay
    u = (rx * ex + ry * ey) * inv
    t = F(0) if u < 0 else (F(1) if u > 1 else u)
    qx, qy = rx - t * ex, ry - t * ey
    d = qx * qx + qy * qy
    R2, E2 = rx * rx + ry * ry, ex * ex + ey * ey
    c = E2 * inv
    b = 2 * EPS + EPS * EPS + g(4) * c
    bound = 2 * (R2 + E2) * (g(2) * (1 + b) ** 2 + 2 * b + b * b)
    return d, bound


def exact_D(px, py, records):
    """(D, bound): the minimum over the records and the largest per-record bound"""
    ds = [exact_d(px, py, rec) for rec in np.asarray(records, dtype=np.float64).reshape(-1, 5)]
    return min(d for d, _ in ds), max(b for _, b in ds)


def exact_p(points_xy, records):
    """(p, bound) of one sample's S points ((S, 2))"""
    pts = np.asarray(points_xy, dtype=np.float64).reshape(-1, 2)
    S = len(pts)
    Ds = [exact_D(x, y, records) for x, y in pts]
    total, err = sum(d for d, _ in Ds), sum(b for _, b in Ds)
    return total / S, err / S + g(S) * (total + err) / S


def adversarial_cases():
    """(name, pose (x, y), path points) — the cases the definition can go wrong on"""
    big, small = 1e7, 1e-3
    return [
        ("on_segment", (0.5, 0.5), [(0.0, 0.0), (1.0, 1.0)]),
        ("on_segment_inexact", (0.1 + 0.3 * 0.7, 0.2 + 0.3 * 0.1), [(0.1, 0.2), (0.8, 0.3)]),
        ("beyond_start", (-2.0, 0.25), [(0.0, 0.0), (1.0, 0.0)]),
        ("beyond_end", (3.0, -0.25), [(0.0, 0.0), (1.0, 0.0)]),
        ("at_vertex", (1.0, 0.0), [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0)]),
        ("one_point", (0.3, -0.4), [(1.0, 2.0)]),
        ("zero_length", (0.3, -0.4), [(1.0, 2.0), (1.0, 2.0)]),
        ("repeated_collinear", (0.75, 0.1), [(0.0, 0.0), (0.5, 0.0), (0.5, 0.0), (1.0, 0.0), (1.0, 0.0), (2.0, 0.0)]),
        ("near_1e7", (big - 1.5, -big + 0.25), [(big - 3.0, -big), (big, -big + 1.0), (big, -big + 1.0)]),
        ("across_1e7", (0.5, 0.5), [(-big, -big), (big, big)]),
        ("near_1e-3", (small * 1.1, small * 0.9), [(small, small), (small * 2, small * 1.5), (small * 3, small)]),
        ("tiny_segment_far_pose", (5.0, 7.0), [(small, small), (small + 2.0 ** -30, small)]),
        ("clamp_edge_u_is_1", (2.0, 1.0), [(0.0, 0.0), (2.0, 0.0)]),
        ("clamp_edge_u_is_0", (0.0, 1.0), [(0.0, 0.0), (2.0, 0.0)]),
    ]


def random_cases(seed, n):
    """n (pose, path) pairs: paths of 1 .. 17 points at three scales, with repeated points now and then"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        scale = (1.0, 1e-3, 1e6)[i % 3]
        k = int(rng.integers(1, 18))
        pts = rng.uniform(-3.0, 3.0, (k, 2)) * scale
        if k > 2 and i % 4 == 0:
            pts[k // 2] = pts[k // 2 - 1]
        out.append((f"random{i}", tuple(rng.uniform(-4.0, 4.0, 2) * scale), pts))
    return out
