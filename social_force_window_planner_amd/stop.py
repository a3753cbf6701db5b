"""The stop check's braking tail (sfw_set_stop_check) restated in numpy: the loop in include/sfw_hip.h, step by step and in
its operation order, vectorised over the samples.  Elementwise operations only, so every product and sum is rounded on its
own as the kernel rounds it (csrc/sfw_kernels.hip sfw_stop_tail_kernel is compiled without contraction).

EXACT LAYER, meant to be compared bit for bit: the velocities, the headings and the tail length — a fixed sequence of +, -, *,
compare — and, where the heading is 0 throughout and there is no lateral velocity (cos = 1, sin = 0), the poses too.  The sign
of a zero velocity is not defined (the device's fmin / fmax order the zeros, a compare does not).
Elsewhere the poses go through numpy's cos and sin, which may differ from the device's in the last bits."""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import numpy as np

from ._abi import SFW_STOP_MAX_STEPS, SFW_STOP_NONE, SFW_STOP_NOT_RUN, SFW_STOP_UNFINISHED  # noqa: F401  (re-exported)


def new_velocity(vg, vi, a_max, dt):
    """computeNewVelocity over arrays (reference sfw_planner.hpp:457-463): both candidates, then the select"""
    step = np.float64(a_max) * np.float64(dt)
    up_c, dn_c = vi + step, vi - step
    up = np.where(vg < up_c, vg, up_c)
    dn = np.where(vg > dn_c, vg, dn_c)
    return np.where((vg - vi) >= 0, up, dn)


def check_arguments(dec, max_steps, reserved=0):
    """what sfw_set_stop_check refuses: ValueError"""
    if any((not math.isfinite(float(d))) or float(d) < 0 for d in dec):
        raise ValueError("a braking limit is not finite or below 0")
    if not 1 <= int(max_steps) <= SFW_STOP_MAX_STEPS:
        raise ValueError("max_steps outside 1 .. SFW_STOP_MAX_STEPS")
    if reserved != 0:
        raise ValueError("reserved must be 0")


def tail(end, dec, dt, max_steps):
    """The tails of n samples.  end: (n, 6) states (x, y, theta, vx, vy, vtheta) behind the last rollout step; dec: (dec_x,
    dec_y, dec_theta).
    -> steps (n,): the tail's length; unfinished (n,): still moving after max_steps steps; vx, vy, vth: (m, n) velocities
    AFTER tail step j; th: (m, n) heading after it — the heading pose j is checked at; x, y: (m, n) pose j.  m = max(steps);
    entries at j >= steps[i] repeat sample i's last state."""
    check_arguments(dec, max_steps)
    end = np.ascontiguousarray(end, dtype=np.float64).reshape(-1, 6)
    x, y, th, vx, vy, vth = (end[:, c].copy() for c in range(6))
    n = len(end)
    dt = np.float64(dt)
    zero = np.zeros(n)
    steps = np.zeros(n, dtype=np.int64)
    rows = []
    j = 0
    with np.errstate(over="ignore", invalid="ignore"):
        while True:
            live = (vx != 0.0) | (vy != 0.0)
            if j == max_steps or not live.any():
                break
            nvx = new_velocity(zero, vx, dec[0], dt)
            nvy = new_velocity(zero, vy, dec[1], dt)
            nvth = new_velocity(zero, vth, dec[2], dt)
            c, s = np.cos(th), np.sin(th)
            lat = nvy != 0.0
            c2, s2 = np.where(lat, np.cos(np.float64(math.pi / 2) + th), 0.0), np.where(lat, np.sin(np.float64(math.pi / 2) + th), 0.0)
            nx = x + (nvx * c + nvy * c2) * dt  # OLD heading, as the rollout
            ny = y + (nvx * s + nvy * s2) * dt
            nth = th + nvth * dt
            x, y, th = np.where(live, nx, x), np.where(live, ny, y), np.where(live, nth, th)
            vx, vy, vth = np.where(live, nvx, vx), np.where(live, nvy, vy), np.where(live, nvth, vth)
            steps += live
            rows.append((x, y, th, vx, vy, vth))
            j += 1
    unfinished = (vx != 0.0) | (vy != 0.0)
    m = len(rows)
    col = [np.array([r[k] for r in rows]).reshape(m, n) for k in range(6)]
    return NS(steps=steps, unfinished=unfinished, x=col[0], y=col[1], th=col[2], vx=col[3], vy=col[4], vth=col[5])


def verdict(steps, unfinished, illegal):
    """(rejected, hit) per sample from illegal (m, n): is tail pose j of sample i illegal (entries at j >= steps[i] are not
    looked at).  hit: the first illegal pose, SFW_STOP_UNFINISHED, or SFW_STOP_NONE"""
    illegal = np.asarray(illegal, dtype=bool)
    m, n = illegal.shape if illegal.ndim == 2 else (0, len(steps))
    seen = illegal.reshape(m, n) & (np.arange(m)[:, None] < np.asarray(steps)[None, :])
    first = np.where(seen.any(axis=0), seen.argmax(axis=0), SFW_STOP_NONE) if m else np.full(n, SFW_STOP_NONE)
    hit = np.where(unfinished, SFW_STOP_UNFINISHED, first)
    return hit != SFW_STOP_NONE, hit
