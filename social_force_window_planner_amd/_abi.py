"""ctypes mirror of include/sfw_hip.h (POD structs + status codes).

Shared by the product binding (planner.py) and by the oracle binding under
oracle/ — the structs are the ABI, not an implementation.
"""
import ctypes as C

SFW_OK = 0
SFW_ERR_INVALID_ARG = -1
SFW_ERR_NO_DEVICE = -2
SFW_ERR_HIP = -3
SFW_ERR_STATE = -4
SFW_ERR_UNSUPPORTED = -5

SFW_COST_INVALID = -1.0
SFW_COST_SKIPPED = -2.0

SFW_PRECISION_F64 = 0
SFW_PRECISION_F32 = 1
SFW_PRECISION_F64_STRICT = 2

SFW_K2_AUTO, SFW_K2_REGISTER, SFW_K2_FLAT = -1, 0, 1
SFW_ORG_NONE, SFW_ORG_REGISTER_1, SFW_ORG_REGISTER_2, SFW_ORG_FLAT = 0, 1, 2, 3


class SfwParams(C.Structure):
    _fields_ = [
        ("max_vel_x", C.c_double),
        ("sim_time", C.c_double),
        ("sim_granularity", C.c_double),
        ("robot_radius", C.c_float),
        ("reserved0", C.c_float),
        ("social_weight", C.c_double),
        ("costmap_weight", C.c_double),
        ("angle_weight", C.c_double),
        ("distance_weight", C.c_double),
        ("vel_weight", C.c_double),
        ("robot_goal_radius", C.c_double),
        ("sfm_force_factor_desired", C.c_double),
        ("sfm_force_factor_obstacle", C.c_double),
        ("sfm_force_sigma_obstacle", C.c_double),
        ("sfm_force_factor_social", C.c_double),
        ("sfm_lambda", C.c_double),
        ("sfm_gamma", C.c_double),
        ("sfm_n", C.c_double),
        ("sfm_n_prime", C.c_double),
        ("sfm_relaxation_time", C.c_double),
        ("sfm_force_factor_group_gaze", C.c_double),
        ("sfm_force_factor_group_coherence", C.c_double),
        ("sfm_force_factor_group_repulsion", C.c_double),
        ("precision", C.c_int32),
        ("reserved1", C.c_int32),
    ]


def default_params(**overrides):
    """ControllerParams defaults (reference sfw_planner.hpp:56-66) plus
    lightsfm's sfm::Parameters defaults."""
    p = SfwParams()
    p.max_vel_x = 0.7
    p.sim_time = 1.0
    p.sim_granularity = 0.025
    p.robot_radius = 0.35
    p.social_weight = 1.2
    p.costmap_weight = 2.0
    p.angle_weight = 0.7
    p.distance_weight = 1.0
    p.vel_weight = 1.0
    p.robot_goal_radius = 0.20
    p.sfm_force_factor_desired = 2.0
    p.sfm_force_factor_obstacle = 10.0
    p.sfm_force_sigma_obstacle = 0.2
    p.sfm_force_factor_social = 2.1
    p.sfm_lambda = 2.0
    p.sfm_gamma = 0.35
    p.sfm_n = 2.0
    p.sfm_n_prime = 3.0
    p.sfm_relaxation_time = 0.5
    p.sfm_force_factor_group_gaze = 3.0
    p.sfm_force_factor_group_coherence = 2.0
    p.sfm_force_factor_group_repulsion = 1.0
    p.precision = SFW_PRECISION_F64
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(f"sfw_params has no field {k!r}")
        setattr(p, k, v)
    return p


class SfwAgent(C.Structure):
    _fields_ = [
        ("x", C.c_double),
        ("y", C.c_double),
        ("vx", C.c_double),
        ("vy", C.c_double),
        ("goal_x", C.c_double),
        ("goal_y", C.c_double),
        ("goal_radius", C.c_double),
        ("desired_velocity", C.c_double),
        ("radius", C.c_double),
        ("has_goal", C.c_int32),
        ("id", C.c_int32),
        ("group_id", C.c_int32),
        ("reserved", C.c_int32),
    ]


class SfwRobotState(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("x", "y", "theta", "vx", "vy", "vtheta")]


class SfwGoalArgs(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("acc_x", "acc_y", "acc_theta", "wpx", "wpy")]


class SfwBest(C.Structure):
    _fields_ = [
        ("index", C.c_int64),
        ("cost", C.c_double),
        ("vx", C.c_double),
        ("vy", C.c_double),
        ("vtheta", C.c_double),
        ("n_valid", C.c_int64),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SfwBestKey(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("cost", "neg_linvel", "abs_angvel", "neg_index")]

    def as_tuple(self):
        return (self.cost, self.neg_linvel, self.abs_angvel, self.neg_index)


class SfwPlanInfo(C.Structure):
    _fields_ = [("split_step", C.c_int32), ("levels", C.c_int32), ("chunks", C.c_int32), ("organisation", C.c_int32),
                ("classes", C.c_int64), ("class_steps", C.c_int64), ("samples", C.c_int64), ("flat_samples", C.c_int64),
                ("one_launch", C.c_int64), ("rest_noise_unreproduced", C.c_int64)]

    def as_dict(self):
        return {"split_step": self.split_step, "levels": self.levels, "chunks": self.chunks, "classes": self.classes,
                "class_steps": self.class_steps, "samples": self.samples, "organisation": self.organisation,
                "flat_samples": self.flat_samples, "one_launch": self.one_launch,
                "rest_noise_unreproduced": self.rest_noise_unreproduced}


# Every symbol include/sfw_hip.h declares (checked by tests/test_abi.py).
EXPORTED_SYMBOLS = (
    "sfw_params_default",
    "sfw_abi_version",
    "sfw_create",
    "sfw_destroy",
    "sfw_set_params",
    "sfw_last_error",
    "sfw_set_costmap",
    "sfw_set_footprint",
    "sfw_set_agents",
    "sfw_score_grid",
    "sfw_score_one",
    "sfw_grid_stage",
    "sfw_grid_launch",
    "sfw_grid_sync",
    "sfw_grid_fetch",
    "sfw_grid_costs_view",
    "sfw_grid_plan_info",
    "sfw_plan_shared_prefix",
    "sfw_plan_shared_prefix_items",
    "sfw_plan_row_blocks",
    "sfw_plan_axis_classes",
    "sfw_set_k2_form",
    "sfw_set_timing",
    "sfw_last_launch_ms",
    "sfw_last_clock_ghz",
    "sfw_grid_points",
    "sfw_grid_points_batch",
    "sfw_set_points_capture",
    "sfw_stream",
    "sfw_multi_create",
    "sfw_multi_destroy",
    "sfw_multi_last_error",
    "sfw_multi_describe",
    "sfw_multi_ranks",
    "sfw_multi_rank_handle",
    "sfw_multi_set_params",
    "sfw_multi_set_costmap",
    "sfw_multi_set_footprint",
    "sfw_multi_set_agents",
    "sfw_multi_score_grid",
    "sfw_multi_rank_rows",
    "sfw_multi_last_us",
    "sfw_multi_grid_points",
    "sfw_batch_create",
    "sfw_batch_destroy",
    "sfw_batch_last_error",
    "sfw_batch_size",
    "sfw_batch_member",
    "sfw_batch_launch",
    "sfw_batch_fetch",
    "sfw_batch_score_grid",
    "sfw_batch_describe",
    "sfw_batch_last_us",
    "sfw_batch_set_list_fusion",
    "sfw_batch_get_list_fusion",
    "sfw_batch_score_samples",
    "sfw_batch_score_sequences",
    "sfw_batch_score_perturbed",
    "sfw_ensemble_set_list_fusion",
    "sfw_ensemble_get_list_fusion",
    "sfw_ensemble_batch_desc",
    "sfw_set_terms_capture",
    "sfw_grid_rescore",
    "sfw_grid_terms",
    "sfw_ensemble_create",
    "sfw_ensemble_destroy",
    "sfw_ensemble_last_error",
    "sfw_ensemble_size",
    "sfw_ensemble_member",
    "sfw_ensemble_set_params",
    "sfw_ensemble_set_costmap",
    "sfw_ensemble_set_footprint",
    "sfw_ensemble_set_hypothesis",
    "sfw_ensemble_score_grid",
    "sfw_ensemble_aggregate",
    "sfw_ensemble_last_us",
    "sfw_samples_stage",
    "sfw_score_samples",
    "sfw_sequences_stage",
    "sfw_score_sequences",
    "sfw_score_one_crowd",
    "sfw_grid_crowd",
    "sfw_grid_blend",
    "sfw_sequences_perturb_stage",
    "sfw_score_perturbed",
    "sfw_sequences_knots",
    "sfw_sequences_normals",
    "sfw_ensemble_score_sequences",
    "sfw_ensemble_score_perturbed",
    "sfw_ensemble_blend",
    "sfw_sequences_control_cost",
    "sfw_grid_blend_control",
    "sfw_mppi_run",
    "sfw_ensemble_blend_control",
    "sfw_ensemble_mppi_run",
    "sfw_ensemble_set_risk",
    "sfw_ensemble_get_risk",
    "sfw_set_footprint_clearance",
    "sfw_footprint_clearance_info",
    "sfw_footprint_clearance_map",
    "sfw_set_stop_check",
    "sfw_get_stop_check",
    "sfw_grid_stop_info",
    "sfw_grid_stop_points",
    "sfw_ensemble_set_stop_check",
    "sfw_set_path",
    "sfw_get_path",
    "sfw_grid_path_term",
    "sfw_grid_rescore_path",
    "sfw_ensemble_set_path",
)
# per-term costs (sfw_set_terms_capture / sfw_grid_rescore / sfw_grid_terms)
SFW_TERM_VEL, SFW_TERM_DISTANCE, SFW_TERM_ANGLE, SFW_TERM_COSTMAP, SFW_TERM_SOCIAL = 0, 1, 2, 3, 4
SFW_N_TERMS = 5
SFW_RESCORE_MAX_K = 1024


class SfwWeights(C.Structure):
    """sfw_weights (include/sfw_hip.h): the five weights of sfw_params in term order."""

    _fields_ = [("vel", C.c_double), ("distance", C.c_double), ("angle", C.c_double), ("costmap", C.c_double),
                ("social", C.c_double)]


# softmin blend (sfw_grid_blend)
SFW_BLEND_MAX_L = 16


class SfwBlendStat(C.Structure):
    """sfw_blend_stat (include/sfw_hip.h): one temperature's record of sfw_grid_blend."""

    _fields_ = [("lambda_", C.c_double), ("j_min", C.c_double), ("eta", C.c_double), ("sum_w2", C.c_double),
                ("n_valid", C.c_int64), ("index_min", C.c_int64)]

    def as_dict(self):
        d = {"lambda": self.lambda_, "j_min": self.j_min, "eta": self.eta, "sum_w2": self.sum_w2, "n_valid": self.n_valid,
             "index_min": self.index_min}
        d["ess"] = self.eta * self.eta / self.sum_w2 if self.sum_w2 > 0.0 else 0.0
        return d


# perturbed sequences (sfw_sequences_perturb_stage)
SFW_SEQ_MAX_KNOTS = 64
SFW_PERTURB_KEEP_NOMINAL, SFW_PERTURB_NO_VY, SFW_PERTURB_KEEP_NORMALS = 1, 2, 4


class SfwPerturb(C.Structure):
    """sfw_perturb (include/sfw_hip.h): what a perturbed stage draws its knots from."""

    _fields_ = [("seed", C.c_uint64), ("nominal", C.c_void_p), ("sigma", C.c_double * 3), ("lo", C.c_double * 3),
                ("hi", C.c_double * 3), ("flags", C.c_int32), ("reserved", C.c_int32)]


# chained MPPI iterations (sfw_mppi_run)
SFW_MPPI_MAX_ITER = 32


class SfwMppi(C.Structure):
    """sfw_mppi (include/sfw_hip.h): iterations, the blend's temperature and the control cost's factor."""

    _fields_ = [("iterations", C.c_int32), ("reserved", C.c_int32), ("lambda_", C.c_double), ("gamma", C.c_double)]


# one grid under several crowd hypotheses (sfw_ensemble_*)
SFW_ENSEMBLE_MAX_M = 64
SFW_ENSEMBLE_MEAN, SFW_ENSEMBLE_MAX = 0, 1


class SfwRisk(C.Structure):
    """sfw_risk (include/sfw_hip.h): the tail mass of the social work's CVaR and the bound on the contact mass."""

    _fields_ = [("tail_mass", C.c_double), ("contact_mass", C.c_double), ("reserved", C.c_int64)]


# the stop check (sfw_set_stop_check)
SFW_STOP_MAX_STEPS = 4096
SFW_STOP_NONE, SFW_STOP_UNFINISHED, SFW_STOP_NOT_RUN = -1, -2, -3


class SfwStopCheck(C.Structure):
    """sfw_stop_check (include/sfw_hip.h): the braking limits and the cap on the tail's length."""

    _fields_ = [("dec_x", C.c_double), ("dec_y", C.c_double), ("dec_theta", C.c_double), ("max_steps", C.c_int32),
                ("reserved", C.c_int32)]


class SfwStopRec(C.Structure):
    """sfw_stop_rec (include/sfw_hip.h): a sample's tail length and its first illegal tail pose (or a SFW_STOP_* sentinel)."""

    _fields_ = [("steps", C.c_int32), ("hit", C.c_int32)]


# the path term (sfw_set_path)
SFW_PATH_MAX_POINTS = 1024
SFW_PATH_MAX_COORD = 1e7


class SfwPath(C.Structure):
    """sfw_path (include/sfw_hip.h): the global plan's points and the path term's weight."""

    _fields_ = [("xy", C.POINTER(C.c_double)), ("n_points", C.c_int32), ("reserved", C.c_int32), ("weight", C.c_double)]


SFW_MULTI_RCCL, SFW_MULTI_HOST_REDUCE = 0, 1
SFW_BATCH_MAX = 256


class SfwBatchDesc(C.Structure):
    """sfw_batch_desc (include/sfw_hip.h): what the last sfw_batch_launch did."""

    _fields_ = [("members", C.c_int32), ("one_launch_members", C.c_int32), ("own_path_members", C.c_int32),
                ("batch_launches", C.c_int32), ("batch_blocks", C.c_int64), ("lds_bytes", C.c_int32)]


class CtrlParams(C.Structure):
    """Numeric ControllerParams (reference sfw_planner.hpp:186-226), the layout of
    sfwh_params in host/sfw_host_capi.cpp."""

    _fields_ = [(n, C.c_double) for n in (
        "max_vel_x", "min_vel_x", "max_vel_th", "min_vel_th", "max_trans_acc", "max_rot_acc",
        "min_in_place_vel_th", "yaw_goal_tolerance", "xy_goal_tolerance", "wp_tolerance", "sim_time",
        "sim_granularity", "robot_radius", "social_weight", "costmap_weight", "angle_weight",
        "distance_weight", "vel_weight")] + [("is_circular", C.c_int32), ("precision", C.c_int32)]


def default_ctrl_params(**overrides):
    """ControllerParams() defaults, reference sfw_planner.hpp:56-66."""
    c = CtrlParams()
    c.max_vel_x, c.min_vel_x = 0.7, 0.1
    c.max_vel_th, c.min_vel_th = 0.5, 0.1
    c.max_trans_acc, c.max_rot_acc = 1.0, 1.0
    c.min_in_place_vel_th = 0.3
    c.yaw_goal_tolerance, c.xy_goal_tolerance, c.wp_tolerance = 0.05, 0.1, 0.5
    c.sim_time, c.sim_granularity = 1.0, 0.025
    c.robot_radius = float(C.c_float(0.35).value)
    c.social_weight, c.costmap_weight, c.angle_weight, c.distance_weight, c.vel_weight = 1.2, 2.0, 0.7, 1.0, 1.0
    c.is_circular, c.precision = 1, SFW_PRECISION_F64
    for k, v in overrides.items():
        if not hasattr(c, k):
            raise AttributeError(f"ControllerParams has no field {k!r}")
        setattr(c, k, v)
    return c


# SFWPlanner::Branch in host/sfw_planner.hpp (which exit of findBestAction ran)
BRANCH_NOT_RUNNING, BRANCH_GOAL_REACHED, BRANCH_ROTATE_IN_PLACE, BRANCH_ROTATE_BLOCKED = 0, 1, 2, 3
BRANCH_APPROACH, BRANCH_GRID, BRANCH_GRID_FAILED = 4, 5, 6
