"""Crowd hypotheses for sfw_ensemble_* (planner.EnsembleScorer).

The reference gives every person one goal, position + naive_goal_time * velocity (reference
src/sensor_interface.cpp:491-502): one velocity estimate projected over one hand-set horizon.  The builders here turn one
agent array into several plausible ones, to be scored together and aggregated on the device.
"""
from __future__ import annotations

import ctypes as C
import math

from ._abi import SfwAgent


def _copy(agents):
    out = (SfwAgent * len(agents))()
    for i, a in enumerate(agents):
        C.memmove(C.byref(out[i]), C.byref(a), C.sizeof(SfwAgent))
    return out


def naive_goal_hypotheses(agents, goal_times, heading_offsets=(0.0,)):
    """One agent array per (goal time t, heading offset d) pair, time outer: every person (index >= 1) gets its velocity
    rotated by d radians and its goal set to pos + t * velocity, as the reference derives it.  The robot (index 0) and every
    other field are copied unchanged; an offset of exactly 0.0 leaves the velocity untouched bit for bit."""
    out = []
    for t in goal_times:
        t = float(t)
        for d in heading_offsets:
            d = float(d)
            hyp = _copy(agents)
            c, s = math.cos(d), math.sin(d)
            for a in list(hyp)[1:]:
                if d != 0.0:
                    a.vx, a.vy = c * a.vx - s * a.vy, s * a.vx + c * a.vy
                a.goal_x = a.x + t * a.vx
                a.goal_y = a.y + t * a.vy
            out.append(hyp)
    return out
