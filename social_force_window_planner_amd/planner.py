"""ctypes binding of the product C-ABI library (libsfw_hip.so, include/sfw_hip.h).

This is plumbing for tests and bench.py; the C++ host mirror of the reference's
SFWPlanner lives in host/.  There is no CPU fallback here: if the HIP library
is missing or no GPU is visible, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from ._abi import (
    EXPORTED_SYMBOLS,
    SFW_ENSEMBLE_MAX,
    SFW_ENSEMBLE_MEAN,
    SFW_ERR_NO_DEVICE,
    SFW_OK,
    SfwAgent,
    SfwBatchDesc,
    SfwBest,
    SfwBestKey,
    SfwBlendStat,
    SFW_BLEND_MAX_L,
    SfwGoalArgs,
    SfwMppi,
    SFW_MPPI_MAX_ITER,
    SfwParams,
    SfwPerturb,
    SfwRisk,
    SfwRobotState,
    SfwPath,
    SfwPlanInfo,
    SfwStopCheck,
    SfwStopRec,
    SfwWeights,
    SFW_N_TERMS,
    default_params,
)

_HERE = os.path.dirname(os.path.abspath(__file__))
# SFW_HIP_LIB: load another build of the same library (A/B kernel tuning in one GPU session;
# boxes differ by ~10 % in sustained clocks, so variants are only comparable within one run)
LIB_PATH = os.environ.get("SFW_HIP_LIB") or os.path.join(_HERE, "libsfw_hip.so")
_lib = None


class SfwError(RuntimeError):
    def __init__(self, status, what, detail=""):
        super().__init__(f"{what} failed: status {status}" + (f" ({detail})" if detail else ""))
        self.status = status


def build(force=False):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles on CPU)."""
    csrc = os.path.join(_HERE, "csrc")
    # (everything the Makefile compiles or includes, and the Makefile itself)
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(_HERE, "..", "include", "sfw_hip.h")]
    stale = (not os.path.exists(LIB_PATH)) or any(
        os.path.getmtime(LIB_PATH) < os.path.getmtime(s) for s in srcs)
    if force or stale:
        r = subprocess.run(["make", "-C", csrc, "all"], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("building libsfw_hip.so failed:\n" + r.stdout + r.stderr)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback for the scoring path)")
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.sfw_params_default.argtypes = [C.POINTER(SfwParams)]
        L.sfw_params_default.restype = None
        L.sfw_abi_version.restype = C.c_int
        L.sfw_create.argtypes = [C.POINTER(SfwParams), C.c_int, C.POINTER(vp)]
        L.sfw_destroy.argtypes = [vp]
        L.sfw_set_params.argtypes = [vp, C.POINTER(SfwParams)]
        L.sfw_last_error.argtypes = [vp]
        L.sfw_last_error.restype = C.c_char_p
        L.sfw_set_costmap.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_double]
        L.sfw_set_footprint.argtypes = [vp, vp, C.c_int32]
        L.sfw_set_agents.argtypes = [vp, vp, C.c_int32, vp, C.c_int32]
        L.sfw_score_grid.argtypes = [vp, C.POINTER(SfwRobotState), vp, C.c_int32, vp, C.c_int32,
                                     C.POINTER(SfwGoalArgs), vp, C.POINTER(SfwBest)]
        L.sfw_score_one.argtypes = [vp, C.POINTER(SfwRobotState), C.c_double, C.c_double, C.c_double,
                                    C.POINTER(SfwGoalArgs), C.POINTER(C.c_double), vp, C.c_int32,
                                    C.POINTER(C.c_int32)]
        L.sfw_grid_stage.argtypes = [vp, C.POINTER(SfwRobotState), vp, C.c_int32, vp, C.c_int32,
                                     C.POINTER(SfwGoalArgs), C.c_int64]
        L.sfw_grid_launch.argtypes = [vp]
        L.sfw_grid_sync.argtypes = [vp]
        L.sfw_grid_fetch.argtypes = [vp, vp, C.POINTER(SfwBest), C.POINTER(SfwBestKey)]
        L.sfw_grid_plan_info.argtypes = [vp, C.POINTER(SfwPlanInfo)]
        L.sfw_set_k2_form.argtypes = [vp, C.c_int32]
        L.sfw_set_timing.argtypes = [vp, C.c_int32]
        L.sfw_last_launch_ms.argtypes = [vp, C.c_int32, C.POINTER(C.c_float)]
        L.sfw_last_clock_ghz.argtypes = [vp, C.POINTER(C.c_double)]
        L.sfw_grid_points.argtypes = [vp, C.c_int64, vp, C.c_int32, C.POINTER(C.c_int32)]
        L.sfw_grid_points_batch.argtypes = [vp, C.c_int64, C.c_int64, vp, vp]
        L.sfw_set_points_capture.argtypes = [vp, C.c_int32]
        L.sfw_stream.argtypes = [vp]
        L.sfw_stream.restype = vp
        L.sfw_multi_create.argtypes = [C.POINTER(SfwParams), C.POINTER(C.c_int), C.c_int32, C.c_int32, C.POINTER(vp)]
        L.sfw_multi_destroy.argtypes = [vp]
        L.sfw_multi_last_error.argtypes = [vp]
        L.sfw_multi_last_error.restype = C.c_char_p
        L.sfw_multi_ranks.argtypes = [vp]
        L.sfw_multi_ranks.restype = C.c_int32
        L.sfw_multi_rank_handle.argtypes = [vp, C.c_int32]
        L.sfw_multi_rank_handle.restype = vp
        L.sfw_multi_set_params.argtypes = [vp, C.POINTER(SfwParams)]
        L.sfw_multi_set_costmap.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_double]
        L.sfw_multi_set_footprint.argtypes = [vp, vp, C.c_int32]
        L.sfw_multi_set_agents.argtypes = [vp, vp, C.c_int32, vp, C.c_int32]
        L.sfw_multi_score_grid.argtypes = [vp, C.POINTER(SfwRobotState), vp, C.c_int32, vp, C.c_int32,
                                           C.POINTER(SfwGoalArgs), vp, C.POINTER(SfwBest)]
        L.sfw_multi_last_us.argtypes = [vp, C.c_int32, C.POINTER(C.c_double)]
        L.sfw_multi_rank_rows.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.sfw_plan_row_blocks.argtypes = [vp, C.c_int32, vp, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double,
                                          C.c_double, C.c_int32, C.c_int32, C.c_int32, vp]
        L.sfw_grid_costs_view.argtypes = [vp]
        L.sfw_grid_costs_view.restype = C.c_void_p
        L.sfw_plan_shared_prefix.argtypes = [vp, C.c_int32, vp, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double,
                                             C.c_double, C.c_int32, C.c_int32, vp, vp, C.c_int32, C.POINTER(C.c_int32)]
        L.sfw_plan_shared_prefix_items.argtypes = L.sfw_plan_shared_prefix.argtypes
        L.sfw_multi_grid_points.argtypes = [vp, C.c_int64, vp, C.c_int32, C.POINTER(C.c_int32)]
        L.sfw_batch_create.argtypes = [C.POINTER(SfwParams), C.c_int, C.c_int32, C.POINTER(vp)]
        L.sfw_batch_destroy.argtypes = [vp]
        L.sfw_batch_last_error.argtypes = [vp]
        L.sfw_batch_last_error.restype = C.c_char_p
        L.sfw_batch_size.argtypes = [vp]
        L.sfw_batch_size.restype = C.c_int32
        L.sfw_batch_member.argtypes = [vp, C.c_int32]
        L.sfw_batch_member.restype = vp
        L.sfw_batch_launch.argtypes = [vp]
        L.sfw_batch_fetch.argtypes = [vp, vp]
        L.sfw_batch_score_grid.argtypes = [vp, vp, vp, C.c_int32, vp, C.c_int32, vp, vp]
        L.sfw_batch_describe.argtypes = [vp, C.POINTER(SfwBatchDesc)]
        L.sfw_batch_last_us.argtypes = [vp, C.c_int32, C.POINTER(C.c_double)]
        L.sfw_set_terms_capture.argtypes = [vp, C.c_int32]
        L.sfw_grid_rescore.argtypes = [vp, C.POINTER(SfwWeights), C.c_int32, C.POINTER(SfwBest), vp]
        L.sfw_grid_terms.argtypes = [vp, C.c_int64, C.c_int64, vp]
        L.sfw_ensemble_create.argtypes = [C.POINTER(SfwParams), C.c_int, C.c_int32, C.POINTER(vp)]
        L.sfw_ensemble_destroy.argtypes = [vp]
        L.sfw_ensemble_last_error.argtypes = [vp]
        L.sfw_ensemble_last_error.restype = C.c_char_p
        L.sfw_ensemble_size.argtypes = [vp]
        L.sfw_ensemble_size.restype = C.c_int32
        L.sfw_ensemble_member.argtypes = [vp, C.c_int32]
        L.sfw_ensemble_member.restype = vp
        L.sfw_ensemble_set_params.argtypes = [vp, C.POINTER(SfwParams)]
        L.sfw_ensemble_set_costmap.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_double]
        L.sfw_ensemble_set_footprint.argtypes = [vp, vp, C.c_int32]
        L.sfw_ensemble_set_hypothesis.argtypes = [vp, C.c_int32, vp, C.c_int32, vp, C.c_int32]
        L.sfw_ensemble_score_grid.argtypes = [vp, C.POINTER(SfwRobotState), vp, C.c_int32, vp, C.c_int32,
                                              C.POINTER(SfwGoalArgs), C.c_int32, vp, vp, vp, C.POINTER(SfwBest)]
        L.sfw_ensemble_aggregate.argtypes = [vp, C.c_int32, vp, vp, vp, C.POINTER(SfwBest)]
        L.sfw_ensemble_last_us.argtypes = [vp, C.c_int32, C.POINTER(C.c_double)]
        L.sfw_samples_stage.argtypes = [vp, C.POINTER(SfwRobotState), vp, vp, vp, C.c_int32, C.POINTER(SfwGoalArgs), C.c_int64]
        L.sfw_score_samples.argtypes = [vp, C.POINTER(SfwRobotState), vp, vp, vp, C.c_int32, C.POINTER(SfwGoalArgs), vp,
                                        C.POINTER(SfwBest)]
        L.sfw_score_one_crowd.argtypes = [vp, C.POINTER(SfwRobotState), C.c_double, C.c_double, C.c_double,
                                          C.POINTER(SfwGoalArgs), C.POINTER(C.c_double), vp, vp, vp, C.c_int32, C.c_int32,
                                          C.POINTER(C.c_int32)]
        L.sfw_grid_crowd.argtypes = [vp, C.c_int64, C.POINTER(C.c_double), vp, vp, vp, C.c_int32, C.c_int32,
                                     C.POINTER(C.c_int32)]
        L.sfw_sequences_stage.argtypes = [vp, C.POINTER(SfwRobotState), vp, vp, vp, C.c_int32, C.c_int32, vp,
                                          C.POINTER(SfwGoalArgs), C.c_int64]
        L.sfw_score_sequences.argtypes = [vp, C.POINTER(SfwRobotState), vp, vp, vp, C.c_int32, C.c_int32, vp,
                                          C.POINTER(SfwGoalArgs), vp, C.POINTER(SfwBest)]
        L.sfw_grid_blend.argtypes = [vp, vp, C.c_int32, vp, C.POINTER(SfwBlendStat), vp, vp]
        L.sfw_sequences_perturb_stage.argtypes = [vp, C.POINTER(SfwRobotState), C.POINTER(SfwPerturb), C.c_int32, C.c_int32, vp,
                                                  C.POINTER(SfwGoalArgs), C.c_int64]
        L.sfw_score_perturbed.argtypes = [vp, C.POINTER(SfwRobotState), C.POINTER(SfwPerturb), C.c_int32, C.c_int32, vp,
                                          C.POINTER(SfwGoalArgs), vp, C.POINTER(SfwBest)]
        L.sfw_sequences_knots.argtypes = [vp, C.c_int64, C.c_int64, vp, vp, vp]
        L.sfw_sequences_normals.argtypes = [vp, C.c_int64, C.c_int64, vp]
        L.sfw_ensemble_score_sequences.argtypes = [vp, C.POINTER(SfwRobotState), vp, vp, vp, C.c_int32, C.c_int32, vp,
                                                   C.POINTER(SfwGoalArgs), C.c_int32, vp, vp, vp, C.POINTER(SfwBest)]
        L.sfw_ensemble_score_perturbed.argtypes = [vp, C.POINTER(SfwRobotState), C.POINTER(SfwPerturb), C.c_int32, C.c_int32, vp,
                                                   C.POINTER(SfwGoalArgs), C.c_int32, vp, vp, vp, C.POINTER(SfwBest)]
        L.sfw_ensemble_blend.argtypes = [vp, vp, C.c_int32, vp, C.POINTER(SfwBlendStat), vp, vp]
        L.sfw_sequences_control_cost.argtypes = [vp, C.c_double, vp]
        L.sfw_grid_blend_control.argtypes = [vp, vp, C.c_int32, C.c_double, vp, C.POINTER(SfwBlendStat), vp, vp]
        L.sfw_mppi_run.argtypes = [vp, C.POINTER(SfwRobotState), C.POINTER(SfwPerturb), C.c_int32, C.c_int32, vp,
                                   C.POINTER(SfwGoalArgs), C.POINTER(SfwMppi), C.POINTER(SfwBlendStat), vp, C.POINTER(SfwBest)]
        L.sfw_ensemble_blend_control.argtypes = [vp, vp, C.c_int32, C.c_double, vp, C.POINTER(SfwBlendStat), vp, vp]
        L.sfw_ensemble_mppi_run.argtypes = [vp, C.POINTER(SfwRobotState), C.POINTER(SfwPerturb), C.c_int32, C.c_int32, vp,
                                            C.POINTER(SfwGoalArgs), C.c_int32, vp, C.POINTER(SfwMppi), C.POINTER(SfwBlendStat), vp,
                                            vp, vp, C.POINTER(SfwBest)]
        L.sfw_ensemble_set_risk.argtypes = [vp, C.POINTER(SfwRisk)]
        L.sfw_ensemble_get_risk.argtypes = [vp, C.POINTER(SfwRisk), C.POINTER(C.c_int32)]
        L.sfw_batch_set_list_fusion.argtypes = [vp, C.c_int32]
        L.sfw_batch_get_list_fusion.argtypes = [vp, C.POINTER(C.c_int32)]
        L.sfw_batch_score_samples.argtypes = [vp, vp, vp, vp, vp, C.c_int32, vp, vp]
        L.sfw_batch_score_sequences.argtypes = [vp, vp, vp, vp, vp, C.c_int32, C.c_int32, vp, vp, vp]
        L.sfw_batch_score_perturbed.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, vp, vp, vp]
        L.sfw_ensemble_set_list_fusion.argtypes = [vp, C.c_int32]
        L.sfw_ensemble_get_list_fusion.argtypes = [vp, C.POINTER(C.c_int32)]
        L.sfw_ensemble_batch_desc.argtypes = [vp, C.POINTER(SfwBatchDesc), C.POINTER(C.c_int64)]
        L.sfw_set_footprint_clearance.argtypes = [vp, C.c_int32]
        L.sfw_footprint_clearance_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.sfw_footprint_clearance_map.argtypes = [vp, vp, C.c_uint64]
        L.sfw_set_stop_check.argtypes = [vp, C.POINTER(SfwStopCheck)]
        L.sfw_get_stop_check.argtypes = [vp, C.POINTER(SfwStopCheck), C.POINTER(C.c_int32)]
        L.sfw_grid_stop_info.argtypes = [vp, C.c_int64, C.c_int64, vp]
        L.sfw_grid_stop_points.argtypes = [vp, C.c_int64, C.c_int64, C.c_int32, vp, vp]
        L.sfw_ensemble_set_stop_check.argtypes = [vp, C.POINTER(SfwStopCheck)]
        L.sfw_set_path.argtypes = [vp, C.POINTER(SfwPath)]
        L.sfw_get_path.argtypes = [vp, vp, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
        L.sfw_grid_path_term.argtypes = [vp, C.c_int64, C.c_int64, vp]
        L.sfw_grid_rescore_path.argtypes = [vp, C.POINTER(SfwWeights), vp, C.c_int32, C.POINTER(SfwBest), vp]
        L.sfw_ensemble_set_path.argtypes = [vp, C.POINTER(SfwPath)]
        _lib = L
    return _lib


def exported_symbols():
    L = lib()
    return {name: hasattr(L, name) for name in EXPORTED_SYMBOLS}


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class _Owner:
    """What the owners of a library object share.  A subclass names the attribute that holds its object (_attr) and the
    library's calls that destroy it and read its last error; members (views of handles the object owns) are closed first."""
    _members = ()

    def close(self):
        if getattr(self, self._attr, None):
            for m in self._members:
                m.close()
            getattr(lib(), self._destroy)(getattr(self, self._attr))
            setattr(self, self._attr, C.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != SFW_OK:
            raise SfwError(rc, what, (getattr(lib(), self._last_error)(getattr(self, self._attr)) or b"").decode())


def _blend(check, fn, fn_control, handle, T, K, lambdas, bias, want_weights, gamma):
    """One blend call marshalled (HipScorer.blend, EnsembleScorer.blend): fn without gamma, fn_control with it, over T samples
    of K knots.  Returns (stats, u[L, K, 3], weights[L, T] or None)."""
    lam = np.ascontiguousarray(np.asarray(lambdas, dtype=np.float64).reshape(-1))
    L = len(lam)
    if L < 1 or L > SFW_BLEND_MAX_L:
        raise ValueError(f"blend: need 1 .. {SFW_BLEND_MAX_L} lambdas, got {L}")
    if not np.all(np.isfinite(lam)) or not np.all(lam > 0.0):
        raise ValueError("blend: every lambda must be finite and > 0")
    b = None
    if bias is not None:
        b = np.ascontiguousarray(np.asarray(bias, dtype=np.float64).reshape(-1))
        if len(b) != T:
            raise ValueError(f"blend: bias must hold one value per sample ({T}), got {len(b)}")
    stats = (SfwBlendStat * L)()
    u = np.zeros((L, K, 3), dtype=np.float64)
    w = np.zeros((L, T), dtype=np.float64) if want_weights else None
    bp, wp = b.ctypes.data if b is not None and T else None, w.ctypes.data if w is not None and T else None
    if gamma is None:
        check(fn(handle, lam.ctypes.data, L, bp, stats, u.ctypes.data, wp), fn.__name__)
    else:
        check(fn_control(handle, lam.ctypes.data, L, float(gamma), bp, stats, u.ctypes.data, wp), fn_control.__name__)
    return [stats[l].as_dict() for l in range(L)], u, w


def _mppi_args(robot_state, n, seed, nominal, sigma, lo, hi, knot_steps, goal_args, iterations, lam, gamma, flags):
    """What both mppi_runs hand the library: (the arguments up to goal_args, those from the sfw_mppi on, K, I, stats, plans,
    and what has to stay alive for the duration of the call)."""
    p, nom, ks = HipScorer._perturb(seed, nominal, sigma, lo, hi, knot_steps, flags)
    rs, ga = SfwRobotState(*robot_state), SfwGoalArgs(*goal_args)
    K, I = nom.shape[0], int(iterations)
    m = SfwMppi(I, 0, float(lam), float(gamma))
    room = min(max(I, 1), SFW_MPPI_MAX_ITER)  # (a refused iteration count writes nothing)
    stats = (SfwBlendStat * room)()
    plans = np.zeros((room, K, 3), dtype=np.float64)
    head = (C.byref(rs), C.byref(p), n, K, ks.ctypes.data if len(ks) else None, C.byref(ga))
    return head, (C.byref(m), stats, plans.ctypes.data), K, I, stats, plans, (p, nom, ks, rs, ga, m)


def _path_arg(xy, weight):
    """(pointer to an sfw_path or None, the array it points into) for sfw_set_path / sfw_ensemble_set_path"""
    if xy is None:
        return None, None
    if isinstance(xy, SfwPath):
        return C.byref(xy), xy
    xy = np.ascontiguousarray(np.asarray(xy, dtype=np.float64).reshape(-1, 2))
    p = SfwPath(xy.ctypes.data_as(C.POINTER(C.c_double)), len(xy), 0, weight)
    p._keep = xy
    return C.byref(p), p


class HipScorer(_Owner):
    """The (v,w) grid scorer on one MI355X.  Method-for-method the same surface
    as the CPU checker's scorer class under oracle/ (which this package never imports)."""

    _attr, _destroy, _last_error = "_h", "sfw_destroy", "sfw_last_error"

    def __init__(self, params: SfwParams | None = None, device: int = 0):
        self.params = params if params is not None else default_params()
        self._h = C.c_void_p()
        rc = lib().sfw_create(C.byref(self.params), device, C.byref(self._h))
        if rc == SFW_ERR_NO_DEVICE:
            raise SfwError(rc, "sfw_create", "no HIP device visible; this library has no CPU fallback")
        if rc != SFW_OK:
            raise SfwError(rc, "sfw_create")
        self._grid = None
        self._n_agents = self._n_staged_agents = 0  # as handed over last / as the last stage uploaded them

    def _mark_staged(self, grid, knots=1):
        """Every stage, by whatever call, ends here: the grid's shape, the knots per sample (what blend sizes its mean by)
        and the agent count that stage uploaded (what grid_crowd sizes its rows by) are recorded in this one place."""
        self._grid = grid
        self._n_knots = knots
        self._n_staged_agents = self._n_agents

    @classmethod
    def _member_view(cls, handle, params, owner):
        """A non-owning view of a handle another object owns (BatchScorer.member): every call but destruction."""
        v = cls.__new__(cls)
        v.params = params
        v._h = C.c_void_p(handle)
        v._grid = None
        v._n_agents = v._n_staged_agents = 0
        v._owner = owner  # (keeps the owner, and so the handle, alive as long as the view)
        return v

    def close(self):
        if getattr(self, "_owner", None) is not None:
            self._h = C.c_void_p()
            return
        super().close()

    # -- world state -------------------------------------------------------
    def set_params(self, params):
        self._check(lib().sfw_set_params(self._h, C.byref(params)), "sfw_set_params")
        self.params = params

    def set_costmap(self, cells, origin_x, origin_y, resolution):
        cells = np.ascontiguousarray(cells, dtype=np.uint8)
        sy, sx = cells.shape
        self._check(lib().sfw_set_costmap(self._h, cells.ctypes.data, sx, sy, origin_x, origin_y, resolution),
                    "sfw_set_costmap")

    def set_footprint(self, xy):
        xy = _f64(xy).reshape(-1, 2)
        self._check(lib().sfw_set_footprint(self._h, xy.ctypes.data if len(xy) else None, len(xy)),
                    "sfw_set_footprint")

    def set_agents(self, agents, obstacles=None):
        n = len(agents)
        obs = _f64(obstacles if obstacles is not None else np.zeros((0, 2))).reshape(-1, 2)
        self._check(lib().sfw_set_agents(self._h, C.addressof(agents) if n else None, n,
                                         obs.ctypes.data if len(obs) else None, len(obs)), "sfw_set_agents")
        self._n_agents = n

    def load_scene(self, scene):
        self.set_costmap(scene.cells, scene.origin_x, scene.origin_y, scene.resolution)
        self.set_footprint(scene.footprint)
        self.set_agents(scene.agents, scene.obstacles)

    # -- scoring -----------------------------------------------------------
    def score_grid(self, robot_state, linvels, angvels, goal_args):
        lin, ang = _f64(linvels), _f64(angvels)
        rs, ga = SfwRobotState(*robot_state), SfwGoalArgs(*goal_args)
        costs = np.empty(len(lin) * len(ang), dtype=np.float64)
        best = SfwBest()
        self._check(lib().sfw_score_grid(self._h, C.byref(rs), lin.ctypes.data, len(lin), ang.ctypes.data,
                                         len(ang), C.byref(ga), costs.ctypes.data, C.byref(best)),
                    "sfw_score_grid")
        self._mark_staged((len(lin), len(ang)))
        return costs, best.as_dict()

    def score_one(self, robot_state, vx_samp, vy_samp, vth_samp, goal_args, points_cap=4096):
        rs, ga = SfwRobotState(*robot_state), SfwGoalArgs(*goal_args)
        cost = C.c_double()
        pts = np.zeros((points_cap, 3), dtype=np.float64)
        n = C.c_int32()
        self._check(lib().sfw_score_one(self._h, C.byref(rs), vx_samp, vy_samp, vth_samp, C.byref(ga),
                                        C.byref(cost), pts.ctypes.data, points_cap, C.byref(n)),
                    "sfw_score_one")
        self._grid = None
        return cost.value, pts[: min(n.value, points_cap)].copy()

    # -- device-resident pipeline -----------------------------------------
    def stage(self, robot_state, linvels, angvels, goal_args, index_base=0):
        lin, ang = _f64(linvels), _f64(angvels)
        rs, ga = SfwRobotState(*robot_state), SfwGoalArgs(*goal_args)
        self._check(lib().sfw_grid_stage(self._h, C.byref(rs), lin.ctypes.data, len(lin), ang.ctypes.data,
                                         len(ang), C.byref(ga), index_base), "sfw_grid_stage")
        self._mark_staged((len(lin), len(ang)))

    # -- sample lists (sfw_samples_stage / sfw_score_samples) ---------------
    @staticmethod
    def _sample_list(vx, vtheta, vy):
        vx, vth = _f64(vx).reshape(-1), _f64(vtheta).reshape(-1)
        vyv = None if vy is None else _f64(vy).reshape(-1)
        if len(vth) != len(vx) or (vyv is not None and len(vyv) != len(vx)):
            raise ValueError("sample list: vx, vy and vtheta must have the same length")
        return vx, vth, vyv

    def stage_samples(self, robot_state, vx, vtheta, goal_args, vy=None, index_base=0):
        """Stage a LIST of samples (vx[t], vy[t], vtheta[t]) — vy=None: all 0 — instead of a grid; launch / fetch / plan_info /
        grid_points_batch / cost_terms / rescore then act on the list, sample index t in list order."""
        vx, vth, vyv = self._sample_list(vx, vtheta, vy)
        rs, ga = SfwRobotState(*robot_state), SfwGoalArgs(*goal_args)
        self._check(lib().sfw_samples_stage(self._h, C.byref(rs), vx.ctypes.data if len(vx) else None,
                                            vyv.ctypes.data if vyv is not None and len(vyv) else None,
                                            vth.ctypes.data if len(vth) else None, len(vx), C.byref(ga), index_base),
                    "sfw_samples_stage")
        self._mark_staged((len(vx), 1))

    def score_samples(self, robot_state, vx, vtheta, goal_args, vy=None):
        """The blocking call over a sample list: (costs[n], best) — best["vy"] is the winner's own vy."""
        vx, vth, vyv = self._sample_list(vx, vtheta, vy)
        rs, ga = SfwRobotState(*robot_state), SfwGoalArgs(*goal_args)
        costs = np.empty(len(vx), dtype=np.float64)
        best = SfwBest()
        self._check(lib().sfw_score_samples(self._h, C.byref(rs), vx.ctypes.data if len(vx) else None,
                                            vyv.ctypes.data if vyv is not None and len(vyv) else None,
                                            vth.ctypes.data if len(vth) else None, len(vx), C.byref(ga),
                                            costs.ctypes.data if len(vx) else None, C.byref(best)), "sfw_score_samples")
        self._mark_staged((len(vx), 1))
        return costs, best.as_dict()

    # -- command sequences (sfw_sequences_stage / sfw_score_sequences) -------
    @staticmethod
    def _sequences(vx, vtheta, knot_steps, vy):
        vx, vth = np.ascontiguousarray(_f64(vx)), np.ascontiguousarray(_f64(vtheta))
        vyv = None if vy is None else np.ascontiguousarray(_f64(vy))
        ks = np.ascontiguousarray(np.asarray(knot_steps, dtype=np.int32).reshape(-1))
        if vx.ndim != 2 or vth.shape != vx.shape or (vyv is not None and vyv.shape != vx.shape) or len(ks) != vx.shape[0]:
            raise ValueError("sequences: vx, vy and vtheta must be (K, n) arrays and knot_steps must hold K steps")
        return vx, vth, vyv, ks

    def stage_sequences(self, robot_state, vx, vtheta, knot_steps, goal_args, vy=None, index_base=0):
        """Stage n command SEQUENCES of K knots: vx / vy / vtheta are (K, n) arrays (vy=None: all 0), knot_steps[k] the Euler
        step at which knot k takes over (knot_steps[0] == 0, strictly ascending).  Everything that acts on a staged list then
        acts on the sequences, sample index t in column order; best carries the winner's FIRST knot."""
        vx, vth, vyv, ks = self._sequences(vx, vtheta, knot_steps, vy)
        rs, ga = SfwRobotState(*robot_state), SfwGoalArgs(*goal_args)
        K, n = vx.shape
        self._check(lib().sfw_sequences_stage(self._h, C.byref(rs), vx.ctypes.data if vx.size else None,
                                              vyv.ctypes.data if vyv is not None and vyv.size else None,
                                              vth.ctypes.data if vth.size else None, n, K, ks.ctypes.data if len(ks) else None,
                                              C.byref(ga), index_base), "sfw_sequences_stage")
        self._mark_staged((n, 1), knots=K)

    def score_sequences(self, robot_state, vx, vtheta, knot_steps, goal_args, vy=None):
        """The blocking call over command sequences: (costs[n], best)."""
        vx, vth, vyv, ks = self._sequences(vx, vtheta, knot_steps, vy)
        rs, ga = SfwRobotState(*robot_state), SfwGoalArgs(*goal_args)
        K, n = vx.shape
        costs = np.empty(n, dtype=np.float64)
        best = SfwBest()
        self._check(lib().sfw_score_sequences(self._h, C.byref(rs), vx.ctypes.data if vx.size else None,
                                              vyv.ctypes.data if vyv is not None and vyv.size else None,
                                              vth.ctypes.data if vth.size else None, n, K, ks.ctypes.data if len(ks) else None,
                                              C.byref(ga), costs.ctypes.data if n else None, C.byref(best)), "sfw_score_sequences")
        self._mark_staged((n, 1), knots=K)
        return costs, best.as_dict()

    # -- perturbed sequences (sfw_sequences_perturb_stage / sfw_score_perturbed) ----
    @staticmethod
    def _perturb(seed, nominal, sigma, lo, hi, knot_steps, flags):
        nom = np.ascontiguousarray(_f64(nominal))
        ks = np.ascontiguousarray(np.asarray(knot_steps, dtype=np.int32).reshape(-1))
        if nom.ndim != 2 or nom.shape[1] != 3 or len(ks) != nom.shape[0]:
            raise ValueError("perturbed: nominal must be a (K, 3) array and knot_steps must hold K steps")
        p = SfwPerturb()
        p.seed = int(seed)
        p.nominal = nom.ctypes.data if nom.size else None
        for name, v in (("sigma", sigma), ("lo", lo), ("hi", hi)):
            setattr(p, name, (C.c_double * 3)(*[float(x) for x in np.asarray(v, dtype=np.float64).reshape(3)]))
        p.flags = int(flags)
        return p, nom, ks  # (nom and ks are kept alive by the caller for the duration of the call)

    def stage_perturbed(self, robot_state, n, seed, nominal, sigma, lo, hi, knot_steps, goal_args, flags=0, index_base=0):
        """Stage n command sequences whose knots the DEVICE draws: knot k, channel c of sample t is
        clamp(nominal[k, c] + sigma[c] * z, lo[c], hi[c]) with z a standard normal that depends on (seed, index_base + t, k, c)
        alone (perturb.reference restates it).  nominal is (K, 3); flags: SFW_PERTURB_*.  A sequence stage in every respect."""
        p, nom, ks = self._perturb(seed, nominal, sigma, lo, hi, knot_steps, flags)
        rs, ga = SfwRobotState(*robot_state), SfwGoalArgs(*goal_args)
        K = nom.shape[0]
        self._check(lib().sfw_sequences_perturb_stage(self._h, C.byref(rs), C.byref(p), n, K, ks.ctypes.data if len(ks) else None,
                                                      C.byref(ga), index_base), "sfw_sequences_perturb_stage")
        self._mark_staged((n, 1), knots=K)

    def score_perturbed(self, robot_state, n, seed, nominal, sigma, lo, hi, knot_steps, goal_args, flags=0):
        """The blocking call over perturbed sequences: (costs[n], best)."""
        p, nom, ks = self._perturb(seed, nominal, sigma, lo, hi, knot_steps, flags)
        rs, ga = SfwRobotState(*robot_state), SfwGoalArgs(*goal_args)
        K = nom.shape[0]
        costs = np.empty(max(n, 0), dtype=np.float64)
        best = SfwBest()
        self._check(lib().sfw_score_perturbed(self._h, C.byref(rs), C.byref(p), n, K, ks.ctypes.data if len(ks) else None,
                                              C.byref(ga), costs.ctypes.data if n > 0 else None, C.byref(best)), "sfw_score_perturbed")
        self._mark_staged((n, 1), knots=K)
        return costs, best.as_dict()

    def knots(self, first, count):
        """The knots of samples [first, first + count) of the staged list or sequences as a (K, 3, count) array (vx, vy, vtheta;
        vy 0.0 for a stage without one) — after a perturbed stage, what the device drew."""
        K = getattr(self, "_n_knots", 1) if self._grid is not None else 1
        out = np.zeros((3, K, max(count, 1)), dtype=np.float64)
        self._check(lib().sfw_sequences_knots(self._h, first, count, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data),
                    "sfw_sequences_knots")
        return np.ascontiguousarray(out.transpose(1, 0, 2))

    def normals(self, first, count):
        """The standard normals of the same range of a perturbed stage staged with SFW_PERTURB_KEEP_NORMALS: (K, 3, count)."""
        K = getattr(self, "_n_knots", 1) if self._grid is not None else 1
        out = np.zeros((K, 3, max(count, 1)), dtype=np.float64)
        self._check(lib().sfw_sequences_normals(self._h, first, count, out.ctypes.data), "sfw_sequences_normals")
        return out

    def prepared(self, robot_state, linvels, angvels, goal_args, index_base=0, zero_copy=False):
        """The blocking call with its arguments marshalled ONCE (a C caller builds its structs once too): step() is
        sfw_grid_stage + sfw_grid_launch + sfw_grid_fetch into the same cost buffer every cycle, three foreign calls and
        nothing else — no numpy array, no ctypes struct is created per call."""
        return PreparedGrid(self, robot_state, linvels, angvels, goal_args, index_base, zero_copy)

    def launch(self):
        self._check(lib().sfw_grid_launch(self._h), "sfw_grid_launch")

    def sync(self):
        self._check(lib().sfw_grid_sync(self._h), "sfw_grid_sync")

    def fetch(self, want_costs=True, out=None):
        """out: a caller-owned float64 buffer of nv * nw doubles the cost vector is written to (a C caller passes the same
        array every cycle; a fresh np.empty of >= 128 KB is an mmap + page faults per call)."""
        nv, nw = self._grid
        if want_costs and out is not None:
            if out.dtype != np.float64 or out.size != nv * nw or not out.flags.c_contiguous:
                raise ValueError("fetch(out=...): need a contiguous float64 array of nv * nw elements")
            costs = out
        else:
            costs = np.empty(nv * nw, dtype=np.float64) if want_costs else None
        best, key = SfwBest(), SfwBestKey()
        self._check(lib().sfw_grid_fetch(self._h, costs.ctypes.data if want_costs else None, C.byref(best),
                                         C.byref(key)), "sfw_grid_fetch")
        return costs, best.as_dict(), key.as_tuple()

    def costs_view(self):
        """sfw_grid_costs_view as a read-only numpy array over the handle's pinned cost vector (valid until the next launch),
        or None when the last launch was not mirrored."""
        p = lib().sfw_grid_costs_view(self._h)
        if not p:
            return None
        nv, nw = self._grid
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(nv * nw,))
        a.flags.writeable = False
        return a

    def plan_info(self):
        """How the staged grid will be launched (shared-prefix split step, classes, chunks)."""
        info = SfwPlanInfo()
        self._check(lib().sfw_grid_plan_info(self._h, C.byref(info)), "sfw_grid_plan_info")
        return info.as_dict()

    def set_k2_form(self, form):
        """SFW_K2_AUTO / SFW_K2_REGISTER / SFW_K2_FLAT: the organisation of the social-force kernel's waves
        (bit-identical results; tests and tuning)."""
        self._check(lib().sfw_set_k2_form(self._h, form), "sfw_set_k2_form")

    def set_timing(self, enabled=True):
        """Per-kernel HIP events for last_launch_ms (off by default: latency path)."""
        self._check(lib().sfw_set_timing(self._h, 1 if enabled else 0), "sfw_set_timing")

    def last_launch_ms(self, which=0):
        ms = C.c_float()
        self._check(lib().sfw_last_launch_ms(self._h, which, C.byref(ms)), "sfw_last_launch_ms")
        return ms.value

    def sustained_clock_ghz(self):
        """Shader clock the last timed launch's social-force kernel ran at (0.0: nothing sampled)."""
        v = C.c_double()
        self._check(lib().sfw_last_clock_ghz(self._h, C.byref(v)), "sfw_last_clock_ghz")
        return v.value

    def set_points_capture(self, enabled=True):
        """Small grids: the scoring launch also leaves the Trajectory points (one D2H per dump, no second rollout)."""
        self._check(lib().sfw_set_points_capture(self._h, 1 if enabled else 0), "sfw_set_points_capture")

    def set_footprint_clearance(self, enabled=True):
        """The footprint check's clearance map (on by default): poses whose whole footprint window is free space skip the
        edge walks.  Off: every pose walks its edges.  Results are bit-identical either way (A/B and tests)."""
        self._check(lib().sfw_set_footprint_clearance(self._h, 1 if enabled else 0), "sfw_set_footprint_clearance")

    def footprint_clearance_info(self):
        """(built, half_width) of the staged grid: whether its footprint checks read a clearance map, and the map's window
        half-width r_c in cells (the window is 2 r_c + 1 cells wide; -1 when the footprint is too large for a map)."""
        built, r = C.c_int32(), C.c_int32()
        self._check(lib().sfw_footprint_clearance_info(self._h, C.byref(built), C.byref(r)), "sfw_footprint_clearance_info")
        return bool(built.value), r.value

    def footprint_clearance_map(self, size_y, size_x):
        """The staged grid's clearance map as a (size_y, size_x) uint8 array: 1 where the whole window is on the map and free."""
        out = np.zeros((size_y, size_x), dtype=np.uint8)
        self._check(lib().sfw_footprint_clearance_map(self._h, out.ctypes.data, out.size), "sfw_footprint_clearance_map")
        return out

    def set_stop_check(self, check=None, *, dec_x=None, dec_y=None, dec_theta=None, max_steps=None):
        """sfw_set_stop_check: reject samples that cannot brake to a stop in front of what lies beyond the rollout (read by the
        next stage).  check: an SfwStopCheck, a (dec_x, dec_y, dec_theta, max_steps) tuple, or None with no keyword: off."""
        if check is None and dec_x is None:
            self._check(lib().sfw_set_stop_check(self._h, None), "sfw_set_stop_check")
            return
        if not isinstance(check, SfwStopCheck):
            check = SfwStopCheck(*check) if check is not None else SfwStopCheck(dec_x, dec_y, dec_theta, max_steps)
        self._check(lib().sfw_set_stop_check(self._h, C.byref(check)), "sfw_set_stop_check")

    def stop_check(self):
        """(dec_x, dec_y, dec_theta, max_steps) of the check in force for the next stage, or None while it is off."""
        c, on = SfwStopCheck(), C.c_int32()
        self._check(lib().sfw_get_stop_check(self._h, C.byref(c), C.byref(on)), "sfw_get_stop_check")
        return (c.dec_x, c.dec_y, c.dec_theta, c.max_steps) if on.value else None

    def stop_info(self, first, count):
        """(steps[count], hit[count]) of the last launch: every sample's tail length and first illegal tail pose (SFW_STOP_*)."""
        rec = np.zeros((count, 2), dtype=np.int32)
        self._check(lib().sfw_grid_stop_info(self._h, first, count, rec.ctypes.data), "sfw_grid_stop_info")
        return rec[:, 0].copy(), rec[:, 1].copy()

    def stop_points(self, first, count, steps_cap):
        """The tail poses of `count` consecutive samples of the staged grid: (points[count, steps_cap, 3], n_steps[count])."""
        pts = np.zeros((count, steps_cap, 3), dtype=np.float64)
        n = np.zeros(count, dtype=np.int32)
        self._check(lib().sfw_grid_stop_points(self._h, first, count, steps_cap, pts.ctypes.data, n.ctypes.data), "sfw_grid_stop_points")
        return pts, n

    def set_path(self, xy=None, weight=0.0):
        """sfw_set_path: the path term over the global plan xy ((n, 2) points) with its weight, read by the next stage; None: off."""
        self._check(lib().sfw_set_path(self._h, _path_arg(xy, weight)[0]), "sfw_set_path")

    def path(self):
        """(xy[n, 2], weight) of the path in force for the next stage, or None while it is off."""
        n, w, on = C.c_int32(), C.c_double(), C.c_int32()
        self._check(lib().sfw_get_path(self._h, None, 0, C.byref(n), C.byref(w), C.byref(on)), "sfw_get_path")
        if not on.value:
            return None
        xy = np.zeros((n.value, 2), dtype=np.float64)
        self._check(lib().sfw_get_path(self._h, xy.ctypes.data, n.value, None, None, None), "sfw_get_path")
        return xy, w.value

    def path_term(self, first=0, count=None):
        """The unweighted path term p of `count` samples of the last launch (sentinels where a sample was rejected or skipped)."""
        if count is None:
            nv, nw = self._grid if self._grid is not None else (0, 0)
            count = max(nv * nw - first, 0)
        out = np.zeros(max(count, 1), dtype=np.float64)
        self._check(lib().sfw_grid_path_term(self._h, first, count, out.ctypes.data), "sfw_grid_path_term")
        return out[:count]

    def rescore_path(self, weights, path_weights=None, K=None, want_costs=False):
        """sfw_grid_rescore_path: the last launch under ONE weight vector (5 values) and K path weights (None: the staged
        weight, K times): (K best dicts, (K, samples) costs or None)."""
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(SFW_N_TERMS))
        pw = None if path_weights is None else np.ascontiguousarray(np.asarray(path_weights, dtype=np.float64).reshape(-1))
        K = len(pw) if pw is not None else (1 if K is None else K)
        best = (SfwBest * max(K, 1))()
        costs = None
        if want_costs and self._grid is not None:
            nv, nw = self._grid
            costs = np.empty((K, nv * nw), dtype=np.float64)
        self._check(lib().sfw_grid_rescore_path(self._h, C.cast(w.ctypes.data, C.POINTER(SfwWeights)),
                                                pw.ctypes.data if pw is not None else None, K, best,
                                                costs.ctypes.data if costs is not None else None), "sfw_grid_rescore_path")
        return [best[k].as_dict() for k in range(K)], costs

    def grid_points_batch(self, first, count, n_steps):
        """Trajectory points of `count` consecutive samples: (points[count, n_steps, 3], n_points[count])."""
        pts = np.zeros((count, n_steps, 3), dtype=np.float64)
        n = np.zeros(count, dtype=np.int32)
        self._check(lib().sfw_grid_points_batch(self._h, first, count, pts.ctypes.data, n.ctypes.data),
                    "sfw_grid_points_batch")
        return pts, n

    def grid_points(self, index, points_cap=4096):
        pts = np.zeros((points_cap, 3), dtype=np.float64)
        n = C.c_int32()
        self._check(lib().sfw_grid_points(self._h, index, pts.ctypes.data, points_cap, C.byref(n)),
                    "sfw_grid_points")
        return pts[: min(n.value, points_cap)].copy()

    # -- the predicted crowd behind a score ----------------------------------
    def _num_steps(self):
        n = int(self.params.sim_time / self.params.sim_granularity + 0.5)  # ref :519-525
        return n if n != 0 else 1

    @staticmethod
    def _crowd_buffers(cap, A):
        """(rows of A slots, at least one byte each: the library refuses a NULL state buffer)"""
        n = max(cap, 1) * max(A, 1)
        return (np.zeros(4 * n, dtype=np.float64)[: 4 * max(cap, 1) * A].reshape(max(cap, 1), A, 4),
                np.zeros(n, dtype=np.float64)[: max(cap, 1) * A].reshape(max(cap, 1), A),
                np.zeros(n, dtype=np.int32)[: max(cap, 1) * A].reshape(max(cap, 1), A))

    @staticmethod
    def _crowd_dict(cost, n, state, work, has_goal):
        m = min(n, state.shape[0])
        return {"cost": cost, "n_steps": n, "state": state[:m].copy(), "work": work[:m].copy(), "has_goal": has_goal[:m].copy()}

    def score_one_crowd(self, robot_state, vx_samp, vy_samp, vth_samp, goal_args, steps_cap=None):
        """sfw_score_one_crowd: one scoreTrajectory call and the pedestrian prediction behind it, as
        dict(cost, n_steps, state[n, A, 4], work[n, A], has_goal[n, A]) — row i is the world after step i, agent 0 the robot."""
        rs, ga = SfwRobotState(*robot_state), SfwGoalArgs(*goal_args)
        A, cap = self._n_agents, steps_cap if steps_cap is not None else self._num_steps()
        state, work, hg = self._crowd_buffers(cap, A)
        cost, n = C.c_double(), C.c_int32()
        self._check(lib().sfw_score_one_crowd(self._h, C.byref(rs), vx_samp, vy_samp, vth_samp, C.byref(ga), C.byref(cost),
                                              state.ctypes.data, work.ctypes.data, hg.ctypes.data, A, cap, C.byref(n)),
                    "sfw_score_one_crowd")
        self._grid = None
        return self._crowd_dict(cost.value, n.value, state, work, hg)

    def grid_crowd(self, index, steps_cap=None):
        """sfw_grid_crowd: the same for sample `index` of the staged grid or list (the winner: best["index"]); read-only for
        the launch."""
        A, cap = self._n_staged_agents, steps_cap if steps_cap is not None else self._num_steps()
        state, work, hg = self._crowd_buffers(cap, A)
        cost, n = C.c_double(), C.c_int32()
        self._check(lib().sfw_grid_crowd(self._h, index, C.byref(cost), state.ctypes.data, work.ctypes.data, hg.ctypes.data,
                                         A, cap, C.byref(n)), "sfw_grid_crowd")
        return self._crowd_dict(cost.value, n.value, state, work, hg)

    # -- per-term costs ------------------------------------------------------
    def set_terms_capture(self, enabled=True):
        """Every grid launch also keeps the five unweighted cost terms of every sample (40 B per sample on the device)."""
        self._check(lib().sfw_set_terms_capture(self._h, 1 if enabled else 0), "sfw_set_terms_capture")

    def cost_terms(self, first=0, count=None):
        """The captured terms of the last launch: float64 (count, 5), columns SFW_TERM_VEL .. SFW_TERM_SOCIAL."""
        if count is None:  # (no grid since sfw_score_one: the library answers SFW_ERR_STATE)
            nv, nw = self._grid if self._grid is not None else (0, 0)
            count = max(nv * nw - first, 0)
        out = np.empty((count, SFW_N_TERMS), dtype=np.float64)
        self._check(lib().sfw_grid_terms(self._h, first, count, out.ctypes.data), "sfw_grid_terms")
        return out

    def rescore(self, weights, want_costs=False):
        """The last launch's grid under K weight vectors ((K, 5) array-like: vel, distance, angle, costmap, social) without
        another rollout: (K best dicts as score_grid returns them, (K, nv * nw) costs or None)."""
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1, SFW_N_TERMS))
        K = w.shape[0]
        best = (SfwBest * max(K, 1))()
        costs = None
        if want_costs and self._grid is not None:
            nv, nw = self._grid
            costs = np.empty((K, nv * nw), dtype=np.float64)
        self._check(lib().sfw_grid_rescore(self._h, C.cast(w.ctypes.data, C.POINTER(SfwWeights)), K, best,
                                           costs.ctypes.data if costs is not None else None), "sfw_grid_rescore")
        return [best[k].as_dict() for k in range(K)], costs

    # -- softmin blend ---------------------------------------------------------
    def blend(self, lambdas, bias=None, want_weights=False, gamma=None):
        """sfw_grid_blend over the last launch (grid, list or sequences): the softmin weights exp(-(J - J_min) / lambda) of
        L temperatures, reduced on the device.  bias: one value per sample added to its cost (None: none).  Returns
        (stats: L dicts with lambda, j_min, eta, sum_w2, ess, n_valid, index_min; u[L, K, 3]: the weighted mean of the
        (vx, vy, vtheta) knots; weights[L, T] or None).  Read-only for the launch.
        gamma (a perturbed stage only): sfw_grid_blend_control — gamma times the control cost of every sample's perturbation
        (control_cost) joins the bias on the device."""
        # (no grid staged through this object, e.g. since sfw_score_one: the library answers SFW_ERR_STATE)
        nv, nw = self._grid if self._grid is not None else (0, 0)
        K = getattr(self, "_n_knots", 1) if self._grid is not None else 64  # (SFW_SEQ_MAX_KNOTS: room for any stage)
        return _blend(self._check, lib().sfw_grid_blend, lib().sfw_grid_blend_control, self._h, nv * nw, K, lambdas, bias,
                      want_weights, gamma)

    # -- MPPI on the device: the control cost, chained iterations ----------------
    def control_cost(self, gamma):
        """sfw_sequences_control_cost of the staged perturbed sequences: gamma * c_t for every sample, c_t = sum over knots and
        channels of (nominal / sigma) * z (mppi.control_cost restates it).  Before or after the launch."""
        n = self._grid[0] if self._grid is not None else 0
        out = np.zeros(max(n, 1), dtype=np.float64)
        self._check(lib().sfw_sequences_control_cost(self._h, float(gamma), out.ctypes.data), "sfw_sequences_control_cost")
        return out[:n]

    def mppi_run(self, robot_state, n, seed, nominal, sigma, lo, hi, knot_steps, goal_args, iterations, lam, gamma, flags=0):
        """sfw_mppi_run: `iterations` times perturb (seed + i) -> score -> control cost -> blend at temperature lam -> new
        nominal, chained on the device behind one wait.  Returns (stats: one dict per iteration; plans[I, K, 3]: the nominal
        plan after every iteration; best of the last iteration).  The scorer is left as after the last iteration's
        score_perturbed."""
        head, tail, K, I, stats, plans, _alive = _mppi_args(robot_state, n, seed, nominal, sigma, lo, hi, knot_steps, goal_args,
                                                            iterations, lam, gamma, flags)
        best = SfwBest()
        self._check(lib().sfw_mppi_run(self._h, *head, *tail, C.byref(best)), "sfw_mppi_run")
        self._mark_staged((n, 1), knots=K)
        return [stats[i].as_dict() for i in range(I)], plans, best.as_dict()


def plan_row_blocks(linvels, angvels, robot_state, goal_args, sim_time, num_steps, n_agents, n_ranks):
    """sfw_plan_row_blocks (host only, no device): row offsets [R + 1] of the contiguous blocks of equal planned work."""
    lin, ang = _f64(linvels), _f64(angvels)
    row0 = np.zeros(n_ranks + 1, dtype=np.int32)
    rc = lib().sfw_plan_row_blocks(lin.ctypes.data, len(lin), ang.ctypes.data, len(ang), robot_state[3], robot_state[5],
                                   goal_args[0], goal_args[2], sim_time, num_steps, n_agents, n_ranks, row0.ctypes.data)
    if rc != SFW_OK:
        raise SfwError(rc, "sfw_plan_row_blocks")
    return row0


def planned_share(linvels, angvels, robot_state, goal_args, sim_time, num_steps, n_agents):
    """Share of the algorithmic sample-steps the plan of this grid would integrate (sfw_plan_shared_prefix_items: the work
    items of each level, host only)."""
    lin, ang = _f64(linvels), _f64(angvels)
    ends, cls, n = np.zeros(64, dtype=np.int32), np.zeros(64, dtype=np.int64), C.c_int32()
    rc = lib().sfw_plan_shared_prefix_items(lin.ctypes.data, len(lin), ang.ctypes.data, len(ang), robot_state[3], robot_state[5],
                                            goal_args[0], goal_args[2], sim_time, num_steps, n_agents, ends.ctypes.data,
                                            cls.ctypes.data, 64, C.byref(n))
    if rc != SFW_OK:
        raise SfwError(rc, "sfw_plan_shared_prefix_items")
    k = min(n.value, 64)
    if k == 0:
        return 1.0
    total = len(lin) * len(ang) * num_steps
    prev, class_steps = 0, 0
    for l in range(k):
        class_steps += int(cls[l]) * int(ends[l] - prev)
        prev = int(ends[l])
    return (class_steps + len(lin) * len(ang) * (num_steps - prev)) / total


def plan_info_of_rank(multi, r):
    """sfw_grid_plan_info of rank r's handle of a MultiScorer (after a score_grid)."""
    info = SfwPlanInfo()
    h = lib().sfw_multi_rank_handle(multi._m, r)
    rc = lib().sfw_grid_plan_info(h, C.byref(info))
    if rc != SFW_OK:
        raise SfwError(rc, "sfw_grid_plan_info")
    return info.as_dict()


class PreparedGrid:
    """See HipScorer.prepared."""

    def __init__(self, scorer, robot_state, linvels, angvels, goal_args, index_base, zero_copy=False):
        self.scorer = scorer
        self.lin, self.ang = _f64(linvels).copy(), _f64(angvels).copy()
        self.rs, self.ga = SfwRobotState(*robot_state), SfwGoalArgs(*goal_args)
        self.costs = np.empty(len(self.lin) * len(self.ang), dtype=np.float64)
        self.best, self.key = SfwBest(), SfwBestKey()
        L = lib()
        self._stage, self._launch, self._fetch = L.sfw_grid_stage, L.sfw_grid_launch, L.sfw_grid_fetch
        self._stage_args = (scorer._h, C.byref(self.rs), self.lin.ctypes.data, len(self.lin), self.ang.ctypes.data, len(self.ang),
                            C.byref(self.ga), index_base)
        self._fetch_args = (scorer._h, self.costs.ctypes.data, C.byref(self.best), C.byref(self.key))
        self._fetch_args_nocost = (scorer._h, None, C.byref(self.best), C.byref(self.key))
        scorer._mark_staged((len(self.lin), len(self.ang)))
        self.zero_copy = zero_copy
        self._view, self._view_ptr, self._view_arr = L.sfw_grid_costs_view, None, None

    def step(self, want_costs=True):
        """Returns (costs — the SAME array every call, or with zero_copy a read-only view of the handle's own —, best, key)."""
        s = self.scorer
        rc = self._stage(*self._stage_args)
        if rc != SFW_OK:
            s._check(rc, "sfw_grid_stage")
        rc = self._launch(s._h)
        if rc != SFW_OK:
            s._check(rc, "sfw_grid_launch")
        if want_costs and self.zero_copy:
            # the vector where the launch's selection kernels left it on the host (sfw_grid_costs_view): no memcpy of it
            rc = self._fetch(*self._fetch_args_nocost)
            if rc != SFW_OK:
                s._check(rc, "sfw_grid_fetch")
            p = self._view(s._h)
            if p:
                if p != self._view_ptr:
                    a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(self.costs.size,))
                    a.flags.writeable = False
                    self._view_ptr, self._view_arr = p, a
                return self._view_arr, self.best.as_dict(), self.key.as_tuple()
            self.zero_copy = False  # (a grid too large for the mirror: copy from here on)
        rc = self._fetch(*(self._fetch_args if want_costs else self._fetch_args_nocost))
        if rc != SFW_OK:
            s._check(rc, "sfw_grid_fetch")
        return (self.costs if want_costs else None), self.best.as_dict(), self.key.as_tuple()

    def relaunch(self):
        """launch + selection fetch of the grid staged last (no stage, no cost vector)."""
        s = self.scorer
        s._check(self._launch(s._h), "sfw_grid_launch")
        s._check(self._fetch(*self._fetch_args_nocost), "sfw_grid_fetch")
        return None, self.best.as_dict(), self.key.as_tuple()


class MultiScorer(_Owner):
    """sfw_multi_*: one process driving one handle per listed device (rows of the grid split over them, one
    RCCL all-reduce(min) of the [R,5] key table).  exchange = SFW_MULTI_HOST_REDUCE lets a device be listed
    more than once (tests on a one-GPU box)."""

    _attr, _destroy, _last_error = "_m", "sfw_multi_destroy", "sfw_multi_last_error"

    def __init__(self, params=None, devices=(0,), exchange=0):
        self.params = params if params is not None else default_params()
        self._m = C.c_void_p()
        devs = (C.c_int * len(devices))(*devices)
        rc = lib().sfw_multi_create(C.byref(self.params), devs, len(devices), exchange, C.byref(self._m))
        if rc != SFW_OK:
            raise SfwError(rc, "sfw_multi_create", (lib().sfw_multi_last_error(None) or b"").decode())
        self.n_ranks = lib().sfw_multi_ranks(self._m)

    def load_scene(self, scene):
        cells = np.ascontiguousarray(scene.cells, dtype=np.uint8)
        sy, sx = cells.shape
        self._check(lib().sfw_multi_set_costmap(self._m, cells.ctypes.data, sx, sy, scene.origin_x, scene.origin_y,
                                                scene.resolution), "sfw_multi_set_costmap")
        xy = _f64(scene.footprint).reshape(-1, 2)
        self._check(lib().sfw_multi_set_footprint(self._m, xy.ctypes.data if len(xy) else None, len(xy)),
                    "sfw_multi_set_footprint")
        obs = _f64(scene.obstacles if scene.obstacles is not None else np.zeros((0, 2))).reshape(-1, 2)
        n = len(scene.agents)
        self._check(lib().sfw_multi_set_agents(self._m, C.addressof(scene.agents) if n else None, n,
                                               obs.ctypes.data if len(obs) else None, len(obs)), "sfw_multi_set_agents")

    def set_params(self, params):
        self._check(lib().sfw_multi_set_params(self._m, C.byref(params)), "sfw_multi_set_params")
        self.params = params

    def score_grid(self, robot_state, linvels, angvels, goal_args, want_costs=True):
        lin, ang = _f64(linvels), _f64(angvels)
        rs, ga = SfwRobotState(*robot_state), SfwGoalArgs(*goal_args)
        costs = np.empty(len(lin) * len(ang), dtype=np.float64) if want_costs else None
        best = SfwBest()
        self._check(lib().sfw_multi_score_grid(self._m, C.byref(rs), lin.ctypes.data, len(lin), ang.ctypes.data,
                                               len(ang), C.byref(ga), costs.ctypes.data if want_costs else None,
                                               C.byref(best)), "sfw_multi_score_grid")
        return costs, best.as_dict()

    def describe(self):
        """sfw_multi_describe: devices, exchange and what the RCCL communicators report about themselves."""
        class Desc(C.Structure):
            _fields_ = [("ranks", C.c_int32), ("exchange", C.c_int32), ("communicators", C.c_int32), ("comm_size", C.c_int32),
                        ("rccl_version", C.c_int32), ("devices", C.c_int32 * 64), ("comm_devices", C.c_int32 * 64),
                        ("rccl_path", C.c_char * 512), ("rccl_found", C.c_char * 64)]

        d = Desc()
        lib().sfw_multi_describe.argtypes = [C.c_void_p, C.c_void_p]
        self._check(lib().sfw_multi_describe(self._m, C.byref(d)), "sfw_multi_describe")
        n = min(d.ranks, 64)
        return {"ranks": d.ranks, "exchange": "rccl" if d.exchange == 0 else "host_reduce", "communicators": d.communicators,
                "comm_size": d.comm_size, "rccl_version": d.rccl_version, "devices": list(d.devices[:n]),
                "comm_devices": list(d.comm_devices[:n]), "rccl_path": d.rccl_path.decode(), "rccl_found": d.rccl_found.decode()}

    def rank_rows(self, r):
        """(first row, rows) of rank r in the last score_grid."""
        a, b = C.c_int32(), C.c_int32()
        self._check(lib().sfw_multi_rank_rows(self._m, r, C.byref(a), C.byref(b)), "sfw_multi_rank_rows")
        return a.value, b.value

    def last_us(self):
        out = []
        for which in range(3):
            v = C.c_double()
            self._check(lib().sfw_multi_last_us(self._m, which, C.byref(v)), "sfw_multi_last_us")
            out.append(v.value)
        return {"enqueue_us": out[0], "exchange_us": out[1], "fetch_us": out[2]}

    def grid_points(self, index, points_cap=4096):
        pts = np.zeros((points_cap, 3), dtype=np.float64)
        n = C.c_int32()
        self._check(lib().sfw_multi_grid_points(self._m, index, pts.ctypes.data, points_cap, C.byref(n)),
                    "sfw_multi_grid_points")
        return pts[: min(n.value, points_cap)].copy()


class BatchScorer(_Owner):
    """B planners on one MI355X whose control cycles are scored together (sfw_batch_*): one launch of the batched cycle
    kernel per kernel variant for the members that qualify, the others on their usual path on the same stream.  Each
    member's results are bit-identical to scoring it alone."""

    _attr, _destroy, _last_error = "_b", "sfw_batch_destroy", "sfw_batch_last_error"

    def __init__(self, params: SfwParams | None = None, device: int = 0, B: int = 1):
        self.params = params if params is not None else default_params()
        self._b = C.c_void_p()
        rc = lib().sfw_batch_create(C.byref(self.params), device, B, C.byref(self._b))
        if rc == SFW_ERR_NO_DEVICE:
            raise SfwError(rc, "sfw_batch_create", "no HIP device visible; this library has no CPU fallback")
        if rc != SFW_OK:
            raise SfwError(rc, "sfw_batch_create")
        self.B = B
        self._members = [HipScorer._member_view(lib().sfw_batch_member(self._b, i), self.params, self) for i in range(B)]

    def member(self, i):
        """Member i as a HipScorer that does not own its handle (world state, staging, single-member scoring, points)."""
        return self._members[i]

    def stage(self, i, robot_state, linvels, angvels, goal_args):
        self._members[i].stage(robot_state, linvels, angvels, goal_args)

    def launch(self):
        self._check(lib().sfw_batch_launch(self._b), "sfw_batch_launch")

    def fetch(self):
        """One wait for the batch: the B selections (dicts), member order."""
        best = (SfwBest * self.B)()
        self._check(lib().sfw_batch_fetch(self._b, best), "sfw_batch_fetch")
        return [b.as_dict() for b in best]

    def _costs(self, i):
        m = self._members[i]
        v = m.costs_view()
        return v.copy() if v is not None else m.fetch()[0]

    def score_grid(self, robot_states, linvels, angvels, goal_args_list):
        """sfw_batch_score_grid: member i scores the grid from robot_states[i] with goal_args_list[i].  A list of
        (costs, best), member order."""
        lin, ang = _f64(linvels), _f64(angvels)
        rs = (SfwRobotState * self.B)(*[SfwRobotState(*r) for r in robot_states])
        ga = (SfwGoalArgs * self.B)(*[SfwGoalArgs(*g) for g in goal_args_list])
        best = (SfwBest * self.B)()
        self._check(lib().sfw_batch_score_grid(self._b, rs, lin.ctypes.data, len(lin), ang.ctypes.data, len(ang), ga, best),
                    "sfw_batch_score_grid")
        for m in self._members:
            m._mark_staged((len(lin), len(ang)))
        return [(self._costs(i), best[i].as_dict()) for i in range(self.B)]

    # -- lists, sequences and perturbed rollouts (sfw_batch_set_list_fusion, sfw_batch_score_samples / _sequences / _perturbed)
    def set_list_fusion(self, enabled=True):
        """The sticky switch (off at creation): members staged with a list, sequences or perturbed rollouts whose own launch
        would be the one-kernel cycle join the batched launch instead of taking their own path.  Same bits either way."""
        self._check(lib().sfw_batch_set_list_fusion(self._b, 1 if enabled else 0), "sfw_batch_set_list_fusion")

    def list_fusion(self):
        v = C.c_int32()
        self._check(lib().sfw_batch_get_list_fusion(self._b, C.byref(v)), "sfw_batch_get_list_fusion")
        return v.value

    def stage_samples(self, i, robot_state, vx, vtheta, goal_args, vy=None):
        self._members[i].stage_samples(robot_state, vx, vtheta, goal_args, vy=vy)

    def stage_sequences(self, i, robot_state, vx, vtheta, knot_steps, goal_args, vy=None):
        self._members[i].stage_sequences(robot_state, vx, vtheta, knot_steps, goal_args, vy=vy)

    def stage_perturbed(self, i, robot_state, n, seed, nominal, sigma, lo, hi, knot_steps, goal_args, flags=0):
        self._members[i].stage_perturbed(robot_state, n, seed, nominal, sigma, lo, hi, knot_steps, goal_args, flags=flags)

    def _fleet(self, robot_states, goal_args_list):
        if len(robot_states) != self.B or len(goal_args_list) != self.B:
            raise ValueError(f"batch score: {len(robot_states)} robot states and {len(goal_args_list)} goal arguments for {self.B} members")
        return ((SfwRobotState * self.B)(*[SfwRobotState(*r) for r in robot_states]),
                (SfwGoalArgs * self.B)(*[SfwGoalArgs(*g) for g in goal_args_list]), (SfwBest * self.B)())

    def _scored_lists(self, best, n, knots):
        for m in self._members:
            m._mark_staged((n, 1), knots=knots)
        return [(self._costs(i), best[i].as_dict()) for i in range(self.B)]

    def score_samples(self, robot_states, vx, vtheta, goal_args_list, vy=None):
        """sfw_batch_score_samples: member i scores its own list vx[i], vy[i], vtheta[i] ((B, n) arrays; vy=None: all 0) from
        robot_states[i] with goal_args_list[i].  A list of (costs, best), member order."""
        vx, vth = np.ascontiguousarray(_f64(vx)), np.ascontiguousarray(_f64(vtheta))
        vyv = None if vy is None else np.ascontiguousarray(_f64(vy))
        if vx.ndim != 2 or vx.shape[0] != self.B or vth.shape != vx.shape or (vyv is not None and vyv.shape != vx.shape):
            raise ValueError("batch score_samples: vx, vy and vtheta must be (B, n) arrays")
        rs, ga, best = self._fleet(robot_states, goal_args_list)
        n = vx.shape[1]
        self._check(lib().sfw_batch_score_samples(self._b, rs, vx.ctypes.data if vx.size else None,
                                                  vyv.ctypes.data if vyv is not None and vyv.size else None,
                                                  vth.ctypes.data if vth.size else None, n, ga, best), "sfw_batch_score_samples")
        return self._scored_lists(best, n, 1)

    def score_sequences(self, robot_states, vx, vtheta, knot_steps, goal_args_list, vy=None):
        """sfw_batch_score_sequences: member i scores its own sequences vx[i] ... ((B, K, n) arrays) under the common
        knot_steps.  A list of (costs, best), member order."""
        vx, vth = np.ascontiguousarray(_f64(vx)), np.ascontiguousarray(_f64(vtheta))
        vyv = None if vy is None else np.ascontiguousarray(_f64(vy))
        ks = np.ascontiguousarray(np.asarray(knot_steps, dtype=np.int32).reshape(-1))
        if vx.ndim != 3 or vx.shape[0] != self.B or vth.shape != vx.shape or (vyv is not None and vyv.shape != vx.shape):
            raise ValueError("batch score_sequences: vx, vy and vtheta must be (B, K, n) arrays")
        rs, ga, best = self._fleet(robot_states, goal_args_list)
        K, n = vx.shape[1], vx.shape[2]
        self._check(lib().sfw_batch_score_sequences(self._b, rs, vx.ctypes.data if vx.size else None,
                                                    vyv.ctypes.data if vyv is not None and vyv.size else None,
                                                    vth.ctypes.data if vth.size else None, n, K,
                                                    ks.ctypes.data if len(ks) else None, ga, best), "sfw_batch_score_sequences")
        return self._scored_lists(best, n, K)

    def score_perturbed(self, robot_states, n, perturbs, knot_steps, goal_args_list):
        """sfw_batch_score_perturbed: member i scores n rollouts the device draws from perturbs[i], a dict of
        HipScorer.stage_perturbed's arguments (seed, nominal, sigma, lo, hi and optionally flags).  A list of (costs, best)."""
        if len(perturbs) != self.B:
            raise ValueError(f"batch score_perturbed: {len(perturbs)} perturbations for {self.B} members")
        made = [HipScorer._perturb(q["seed"], q["nominal"], q["sigma"], q["lo"], q["hi"], knot_steps, q.get("flags", 0)) for q in perturbs]
        pt = (SfwPerturb * self.B)(*[m[0] for m in made])
        ks = made[0][2]
        K = made[0][1].shape[0]
        rs, ga, best = self._fleet(robot_states, goal_args_list)
        self._check(lib().sfw_batch_score_perturbed(self._b, rs, pt, n, K, ks.ctypes.data if len(ks) else None, ga, best),
                    "sfw_batch_score_perturbed")
        return self._scored_lists(best, n, K)

    def describe(self):
        d = SfwBatchDesc()
        self._check(lib().sfw_batch_describe(self._b, C.byref(d)), "sfw_batch_describe")
        return {n: getattr(d, n) for n, _ in SfwBatchDesc._fields_}

    def last_us(self):
        """Host wall-clock of the last calls: stage (score_grid only), enqueue, wait + fetch (microseconds)."""
        out = {}
        for which, name in enumerate(("stage", "enqueue", "wait_fetch")):
            v = C.c_double()
            self._check(lib().sfw_batch_last_us(self._b, which, C.byref(v)), "sfw_batch_last_us")
            out[name] = v.value
        return out


_ENSEMBLE_MODES = {"mean": SFW_ENSEMBLE_MEAN, "max": SFW_ENSEMBLE_MAX}


class EnsembleScorer(_Owner):
    """One robot's grid under M crowd hypotheses (sfw_ensemble_*): every hypothesis is scored as a standalone handle would
    score it, in one batch launch, and the per-sample social work is aggregated on the device — "mean" (probability-weighted
    sum, probs default 1/M each) or "max" (worst case).  A sample any hypothesis rejects is rejected; `rejected` counts the
    hypotheses that reject each sample."""

    _attr, _destroy, _last_error = "_e", "sfw_ensemble_destroy", "sfw_ensemble_last_error"

    def __init__(self, params: SfwParams | None = None, device: int = 0, M: int = 1):
        self.params = params if params is not None else default_params()
        self._e = C.c_void_p()
        rc = lib().sfw_ensemble_create(C.byref(self.params), device, M, C.byref(self._e))
        if rc == SFW_ERR_NO_DEVICE:
            raise SfwError(rc, "sfw_ensemble_create", "no HIP device visible; this library has no CPU fallback")
        if rc != SFW_OK:
            raise SfwError(rc, "sfw_ensemble_create")
        self.M = M
        self._grid = None
        self._members = [HipScorer._member_view(lib().sfw_ensemble_member(self._e, m), self.params, self) for m in range(M)]

    def member(self, m):
        """Hypothesis m's handle as a HipScorer that does not own it (its costs, captured terms, points)."""
        return self._members[m]

    # -- world state -------------------------------------------------------
    def set_params(self, params):
        self._check(lib().sfw_ensemble_set_params(self._e, C.byref(params)), "sfw_ensemble_set_params")
        self.params = params
        for m in self._members:
            m.params = params

    def set_costmap(self, cells, origin_x, origin_y, resolution):
        cells = np.ascontiguousarray(cells, dtype=np.uint8)
        sy, sx = cells.shape
        self._check(lib().sfw_ensemble_set_costmap(self._e, cells.ctypes.data, sx, sy, origin_x, origin_y, resolution),
                    "sfw_ensemble_set_costmap")

    def set_footprint(self, xy):
        xy = _f64(xy).reshape(-1, 2)
        self._check(lib().sfw_ensemble_set_footprint(self._e, xy.ctypes.data if len(xy) else None, len(xy)),
                    "sfw_ensemble_set_footprint")

    def set_hypothesis(self, m, agents, obstacles=None):
        n = len(agents)
        obs = _f64(obstacles if obstacles is not None else np.zeros((0, 2))).reshape(-1, 2)
        self._check(lib().sfw_ensemble_set_hypothesis(self._e, m, C.addressof(agents) if n else None, n,
                                                      obs.ctypes.data if len(obs) else None, len(obs)),
                    "sfw_ensemble_set_hypothesis")
        self._members[m]._n_agents = n

    def load_scene(self, scene, hypotheses):
        """The scene's costmap and footprint, and hypotheses[m] = agents or (agents, obstacles) for every member (plain
        agents take the scene's laser points)."""
        if len(hypotheses) != self.M:
            raise ValueError(f"load_scene: {len(hypotheses)} hypotheses for an ensemble of {self.M}")
        self.set_costmap(scene.cells, scene.origin_x, scene.origin_y, scene.resolution)
        self.set_footprint(scene.footprint)
        for m, h in enumerate(hypotheses):
            agents, obs = h if isinstance(h, tuple) else (h, scene.obstacles)
            self.set_hypothesis(m, agents, obs)

    # -- scoring -----------------------------------------------------------
    @staticmethod
    def _mode(mode):
        return _ENSEMBLE_MODES[mode] if isinstance(mode, str) else int(mode)

    def _probs(self, probs):
        return None if probs is None else _f64(probs).reshape(-1)

    def _outputs(self, grid=None):
        nv, nw = self._grid if grid is None else grid
        return np.empty(nv * nw, dtype=np.float64), np.empty(nv * nw, dtype=np.int32), SfwBest()

    def _mark_scored(self, grid, knots=1):
        """Every score that succeeded ends here: the shape aggregate() and blend() size their outputs by, and the members'
        views staged with the same samples (their cost_terms(), knots() and grid_crowd() then work)."""
        self._grid = grid
        self._n_knots = knots
        for m in self._members:
            m._mark_staged(grid, knots=knots)

    def _checked_probs(self, probs, what):
        p = self._probs(probs)
        if p is not None and p.size != self.M:
            raise ValueError(f"{what}: {p.size} probabilities for an ensemble of {self.M}")
        return p

    def score_grid(self, robot_state, linvels, angvels, goal_args, mode="mean", probs=None):
        """(costs, rejected, best): the ensemble cost vector, the hypotheses rejecting each sample, the selection."""
        lin, ang = _f64(linvels), _f64(angvels)
        rs, ga = SfwRobotState(*robot_state), SfwGoalArgs(*goal_args)
        p = self._checked_probs(probs, "score_grid")
        grid = (len(lin), len(ang))
        costs, rejected, best = self._outputs(grid)
        self._check(lib().sfw_ensemble_score_grid(self._e, C.byref(rs), lin.ctypes.data, len(lin), ang.ctypes.data, len(ang),
                                                  C.byref(ga), self._mode(mode), p.ctypes.data if p is not None else None,
                                                  costs.ctypes.data, rejected.ctypes.data, C.byref(best)),
                    "sfw_ensemble_score_grid")
        self._mark_scored(grid)
        return costs, rejected, best.as_dict()

    def score_sequences(self, robot_state, vx, vtheta, knot_steps, goal_args, vy=None, mode="mean", probs=None):
        """n command sequences of K knots ((K, n) arrays as HipScorer.score_sequences takes them; K == 1: a sample list) under
        every hypothesis: (costs[n], rejected[n], best) — best carries the winner's first knot."""
        vx, vth, vyv, ks = HipScorer._sequences(vx, vtheta, knot_steps, vy)
        rs, ga = SfwRobotState(*robot_state), SfwGoalArgs(*goal_args)
        p = self._checked_probs(probs, "score_sequences")
        K, n = vx.shape
        costs, rejected, best = self._outputs((n, 1))
        self._check(lib().sfw_ensemble_score_sequences(self._e, C.byref(rs), vx.ctypes.data if vx.size else None,
                                                       vyv.ctypes.data if vyv is not None and vyv.size else None,
                                                       vth.ctypes.data if vth.size else None, n, K,
                                                       ks.ctypes.data if len(ks) else None, C.byref(ga), self._mode(mode),
                                                       p.ctypes.data if p is not None else None, costs.ctypes.data if n else None,
                                                       rejected.ctypes.data if n else None, C.byref(best)),
                    "sfw_ensemble_score_sequences")
        self._mark_scored((n, 1), knots=K)
        return costs, rejected, best.as_dict()

    def score_perturbed(self, robot_state, n, seed, nominal, sigma, lo, hi, knot_steps, goal_args, flags=0, mode="mean",
                        probs=None):
        """n sequences whose knots the device draws (HipScorer.score_perturbed's arguments; every member holds the same
        knots): (costs[n], rejected[n], best)."""
        pt, nom, ks = HipScorer._perturb(seed, nominal, sigma, lo, hi, knot_steps, flags)
        rs, ga = SfwRobotState(*robot_state), SfwGoalArgs(*goal_args)
        p = self._checked_probs(probs, "score_perturbed")
        K = nom.shape[0]
        costs, rejected, best = self._outputs((max(n, 0), 1))
        self._check(lib().sfw_ensemble_score_perturbed(self._e, C.byref(rs), C.byref(pt), n, K, ks.ctypes.data if len(ks) else None,
                                                       C.byref(ga), self._mode(mode), p.ctypes.data if p is not None else None,
                                                       costs.ctypes.data if n > 0 else None,
                                                       rejected.ctypes.data if n > 0 else None, C.byref(best)),
                    "sfw_ensemble_score_perturbed")
        self._mark_scored((n, 1), knots=K)
        return costs, rejected, best.as_dict()

    def aggregate(self, mode="mean", probs=None):
        """The last score (grid, sequences or perturbed) re-aggregated under another mode / probabilities, no rollout:
        (costs, rejected, best)."""
        p = self._checked_probs(probs, "aggregate")
        # (nothing scored: the library answers SFW_ERR_STATE)
        costs, rejected, best = self._outputs(self._grid if self._grid is not None else (0, 0))
        self._check(lib().sfw_ensemble_aggregate(self._e, self._mode(mode), p.ctypes.data if p is not None else None,
                                                 costs.ctypes.data, rejected.ctypes.data, C.byref(best)),
                    "sfw_ensemble_aggregate")
        return costs, rejected, best.as_dict()

    def blend(self, lambdas, bias=None, want_weights=False, gamma=None):
        """sfw_ensemble_blend: HipScorer.blend over the ENSEMBLE cost vector of the last aggregation and member 0's knots —
        (stats, u[L, K, 3], weights[L, n] or None).
        gamma (after score_perturbed or mppi_run only): sfw_ensemble_blend_control — gamma times the control cost of every
        sample's perturbation joins the bias on the device."""
        nv, nw = self._grid if self._grid is not None else (0, 0)  # (nothing scored: the library answers SFW_ERR_STATE)
        return _blend(self._check, lib().sfw_ensemble_blend, lib().sfw_ensemble_blend_control, self._e, nv * nw,
                      getattr(self, "_n_knots", 1), lambdas, bias, want_weights, gamma)

    def mppi_run(self, robot_state, n, seed, nominal, sigma, lo, hi, knot_steps, goal_args, iterations, lam, gamma, flags=0,
                 mode="mean", probs=None, want_costs=False):
        """sfw_ensemble_mppi_run: HipScorer.mppi_run under every hypothesis — `iterations` times perturb (seed + i) -> score all
        members -> aggregate -> control cost -> blend at temperature lam -> new nominal, chained on the device behind one wait.
        Returns (stats: one dict per iteration; plans[I, K, 3]; best of the last iteration), and with want_costs also the last
        iteration's costs[n] and rejected[n].  The ensemble is left as after the last iteration's score_perturbed."""
        head, tail, K, I, stats, plans, _alive = _mppi_args(robot_state, n, seed, nominal, sigma, lo, hi, knot_steps, goal_args,
                                                            iterations, lam, gamma, flags)
        p = self._checked_probs(probs, "mppi_run")
        costs, rejected, best = self._outputs((max(n, 0), 1))
        out = want_costs and n > 0
        self._check(lib().sfw_ensemble_mppi_run(self._e, *head, self._mode(mode), p.ctypes.data if p is not None else None, *tail,
                                                costs.ctypes.data if out else None, rejected.ctypes.data if out else None,
                                                C.byref(best)), "sfw_ensemble_mppi_run")
        self._mark_scored((n, 1), knots=K)
        res = ([stats[i].as_dict() for i in range(I)], plans, best.as_dict())
        return res + (costs, rejected) if want_costs else res

    # -- risk ---------------------------------------------------------------
    def set_stop_check(self, check=None):
        """sfw_ensemble_set_stop_check: the stop check of every member (an SfwStopCheck or a (dec_x, dec_y, dec_theta,
        max_steps) tuple; None: off)."""
        if check is not None and not isinstance(check, SfwStopCheck):
            check = SfwStopCheck(*check)
        self._check(lib().sfw_ensemble_set_stop_check(self._e, None if check is None else C.byref(check)), "sfw_ensemble_set_stop_check")

    def set_path(self, xy=None, weight=0.0):
        """sfw_ensemble_set_path: the path term of every member ((n, 2) points and the weight; None: off)."""
        self._check(lib().sfw_ensemble_set_path(self._e, _path_arg(xy, weight)[0]), "sfw_ensemble_set_path")

    def set_risk(self, tail_mass=1.0, contact_mass=0.0):
        """sfw_ensemble_set_risk: from here on every aggregation (the score calls, aggregate, mppi_run) takes "mean" as the
        tail expectation of the social work over the worst `tail_mass` of the accepted probability mass, and rejects a sample
        only when more than `contact_mass` of the probability mass ends in contact.  The last score stays: aggregate()
        re-aggregates it under the new setting."""
        r = SfwRisk(float(tail_mass), float(contact_mass), 0)
        self._check(lib().sfw_ensemble_set_risk(self._e, C.byref(r)), "sfw_ensemble_set_risk")

    def clear_risk(self):
        """Back to the plain aggregation (sfw_ensemble_set_risk with NULL)."""
        self._check(lib().sfw_ensemble_set_risk(self._e, None), "sfw_ensemble_set_risk")

    def risk(self):
        """The setting as {"tail_mass", "contact_mass"}, or None while no risk is set."""
        r, on = SfwRisk(), C.c_int32()
        self._check(lib().sfw_ensemble_get_risk(self._e, C.byref(r), C.byref(on)), "sfw_ensemble_get_risk")
        return {"tail_mass": r.tail_mass, "contact_mass": r.contact_mass} if on.value else None

    def knots(self, first, count):
        """The knots of samples [first, first + count) of the last sequence score as (K, 3, count): member 0's (every member
        holds the same)."""
        return self._members[0].knots(first, count)

    # -- list fusion ----------------------------------------------------------
    def set_list_fusion(self, enabled=True):
        """sfw_ensemble_set_list_fusion (off at creation): score_sequences, score_perturbed and every iteration of mppi_run
        score the M members in one batched launch instead of M.  Same bits either way."""
        self._check(lib().sfw_ensemble_set_list_fusion(self._e, 1 if enabled else 0), "sfw_ensemble_set_list_fusion")

    def list_fusion(self):
        v = C.c_int32()
        self._check(lib().sfw_ensemble_get_list_fusion(self._e, C.byref(v)), "sfw_ensemble_get_list_fusion")
        return v.value

    def batch_desc(self):
        """What the private batch's last launch did (BatchScorer.describe's dict) plus "table_uploads": the member-table
        uploads of the last mppi_run's launches."""
        d, up = SfwBatchDesc(), C.c_int64()
        self._check(lib().sfw_ensemble_batch_desc(self._e, C.byref(d), C.byref(up)), "sfw_ensemble_batch_desc")
        out = {n: getattr(d, n) for n, _ in SfwBatchDesc._fields_}
        out["table_uploads"] = up.value
        return out

    def last_us(self):
        """Host wall-clock of the last calls: stage (the score calls only), enqueue, wait + copies out (microseconds)."""
        out = {}
        for which, name in enumerate(("stage", "enqueue", "wait_fetch")):
            v = C.c_double()
            self._check(lib().sfw_ensemble_last_us(self._e, which, C.byref(v)), "sfw_ensemble_last_us")
            out[name] = v.value
        return out
