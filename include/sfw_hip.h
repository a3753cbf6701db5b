/*
 * sfw_hip.h — C ABI of the MI355X-native DWA rollout + social-force scorer.
 *
 * This is the drop-in boundary for ONE hot path of
 * robotics-upo/social_force_window_planner: the (v,w) sample loop of
 * SFWPlanner::findBestAction (reference src/sfw_planner.cpp:338-417) and the
 * two single-sample calls of SFWPlanner::scoreTrajectory
 * (src/sfw_planner.cpp:204-206 and :299-301; signature
 * include/social_force_window_planner/sfw_planner.hpp:309-314).
 *
 * Plain C: POD structs, plain pointers and sizes, int status codes, no C++
 * types and no exceptions across the boundary.  All floating point inputs are
 * double, as in the reference; the two places where the reference computes in
 * float (robot_radius_, normalizeAngle) are float here too.
 *
 * Ownership: the caller owns every buffer it passes in; the library copies
 * what it needs into its own pinned/device buffers during the call.  Output
 * buffers are caller-allocated.
 *
 * Threading: one handle = one planner = one caller thread at a time (the
 * reference holds configuration_mutex_ for the whole findBestAction,
 * src/sfw_planner.cpp:123-454).  Each handle owns one HIP stream.
 *
 * Error convention: every function returns SFW_OK (0) or a negative
 * sfw_status.  An invalid trajectory is DATA, not an error: its cost is
 * exactly -1.0 (src/sfw_planner.cpp:549,561,572,625), never NaN.  Non-finite
 * inputs (agents, laser points, robot state, goal arguments, sample
 * velocities) are refused with SFW_ERR_INVALID_ARG, so no NaN reaches a cost.
 */
#ifndef SFW_HIP_H_
#define SFW_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFW_ABI_VERSION 2 /* 2 (round 6): sfw_plan_info.one_launch, sfw_plan_axis_classes */

typedef enum sfw_status {
  SFW_OK = 0,
  SFW_ERR_INVALID_ARG = -1,  /* null pointer, negative size, ...            */
  SFW_ERR_NO_DEVICE = -2,    /* no HIP device / kernels cannot be launched  */
  SFW_ERR_HIP = -3,          /* a HIP runtime call failed (see last_error)  */
  SFW_ERR_STATE = -4,        /* call order violated (e.g. no costmap set)   */
  SFW_ERR_UNSUPPORTED = -5   /* input does not fit the device (e.g. LDS)     */
} sfw_status;

/* Cost sentinels written into the per-sample cost vector. */
#define SFW_COST_INVALID (-1.0) /* reference "return -1.0"                    */
#define SFW_COST_SKIPPED (-2.0) /* the (0,0) sample the grid loop never scores
                                   (src/sfw_planner.cpp:349-352)             */

/* Robot agent id for callers that have none to give (the reference never sets
 * agents_[0].id, src/sensor_interface.cpp:31-37): no people_msgs tag parses to
 * it, so no person's robot-induced social work is skipped by an id collision. */
#define SFW_ROBOT_ID_NONE INT32_MIN

/* Arithmetic mode of the social-force kernel. */
#define SFW_PRECISION_F64 0 /* parity mode: everything in double            */
#define SFW_PRECISION_F32 1 /* fast mode: agent state, integration and every
                               threshold stay double; only the pair/obstacle
                               FORCES are evaluated in float  */
#define SFW_PRECISION_F64_STRICT 2 /* everything in double as SFW_PRECISION_F64,
                               with the angle's polynomial one degree longer
                               (asin 8 / exp 9 against the default's 7 / 9 —
                               7 / 8 until round 4 —: the pair term at ~1e-14
                               relative instead of ~5e-14; K2 +1 %).  Kept for
                               callers that selected it; since the default
                               evaluates the exponential at degree 9 the two
                               are within a digit of each other */

/*
 * Scoring parameters = the subset of ControllerParams
 * (sfw_planner.hpp:55-66,186-226) that scoreTrajectory reads, plus lightsfm's
 * sfm::Parameters (never overridden by the reference).
 * Fill with sfw_params_default() and then override.
 */
typedef struct sfw_params {
  double max_vel_x;        /* max_trans_vel, 0.7  (:58, used at :654)       */
  double sim_time;         /* 1.0   (:61, :519)                             */
  double sim_granularity;  /* 0.025 (:61, :519)                             */
  float robot_radius;      /* 0.35, FLOAT on purpose (:62,:208, :617)       */
  float reserved0;
  double social_weight;    /* 1.2 (:65)                                     */
  double costmap_weight;   /* 2.0                                           */
  double angle_weight;     /* 0.7                                           */
  double distance_weight;  /* 1.0 (:66)                                     */
  double vel_weight;       /* 1.0                                           */
  double robot_goal_radius; /* 0.20, the per-step robot goal (:608)         */
  /* lightsfm sfm::Parameters defaults */
  double sfm_force_factor_desired;  /* 2.0  */
  double sfm_force_factor_obstacle; /* 10.0 */
  double sfm_force_sigma_obstacle;  /* 0.2  */
  double sfm_force_factor_social;   /* 2.1  */
  double sfm_lambda;                /* 2.0  */
  double sfm_gamma;                 /* 0.35 */
  double sfm_n;                     /* 2.0  */
  double sfm_n_prime;               /* 3.0  */
  double sfm_relaxation_time;       /* 0.5  */
  double sfm_force_factor_group_gaze;      /* 3.0 */
  double sfm_force_factor_group_coherence; /* 2.0 */
  double sfm_force_factor_group_repulsion; /* 1.0 */
  int32_t precision;                /* SFW_PRECISION_*                      */
  int32_t reserved1;
} sfw_params;

/*
 * One social agent = the fields of sfm::Agent the hot path consumes
 * (built by SFMSensorInterface, src/sensor_interface.cpp:31-37,442-527,
 * 552-580).  Index 0 of the array handed to sfw_set_agents is the robot
 * (src/sfw_planner.cpp:155).
 */
typedef struct sfw_agent {
  double x, y;             /* position                                      */
  double vx, vy;           /* velocity; for the robot this is the ROBOT-LOCAL
                              twist, as in sensor_interface.cpp:566-575     */
  double goal_x, goal_y;   /* goals.front().center (ignored if !has_goal)   */
  double goal_radius;      /* goals.front().radius                          */
  double desired_velocity; /* Agent::desiredVelocity.  <= 0 is accepted, as
                              the reference accepts people_velocity_ = 0
                              (sensor_interface.cpp:503): the speed clamp of
                              updatePosition pins a person with 0 where it
                              stands.  Next to a robot without twist it is
                              at exact relative rest at EVERY step, where
                              lightsfm's sign(theta) is the rounding noise of
                              two atan2 (-1, 0 or +1): reproduced for the
                              handed-over state and for a robot that stands
                              still from the start (the linvel = 0 samples),
                              NOT for one that brakes to a stop during the
                              rollout — the angular term of that pair is 0
                              from there on                  */
  double radius;           /* Agent::radius                                 */
  int32_t has_goal;        /* goals non-empty (people: 1, robot at t0: 0)   */
  int32_t id;              /* Agent::id — the robot-on-person force skips a
                              person whose id equals the robot's            */
  int32_t group_id;        /* Agent::groupId (people_msgs tags[1]); < 0 = no
                              group.  Members of a group of >= 2 agents feel
                              lightsfm's gaze/coherence/repulsion forces    */
  int32_t reserved;
} sfw_agent;

/* Robot pose and velocity as findBestAction hands them to scoreTrajectory.
 * The reference truncates all six to float first (src/sfw_planner.cpp:145-152)
 * — the host mirror does that; the ABI takes whatever it is given. */
typedef struct sfw_robot_state {
  double x, y, theta;
  double vx, vy, vtheta;
} sfw_robot_state;

/* Per-call sample-independent arguments of scoreTrajectory. */
typedef struct sfw_goal_args {
  double acc_x, acc_y, acc_theta; /* max_trans_acc_, 0.0, max_rot_acc_      */
  double wpx, wpy;                /* current way-point                      */
} sfw_goal_args;

/* Result of the selection rule (src/sfw_planner.cpp:394-414, :426-468). */
typedef struct sfw_best {
  int64_t index;    /* iv*nw+iw of the winner (a sample list: t), -1 if no sample is selectable */
  double cost;      /* winner's cost, -1.0 if none                           */
  double vx, vy, vtheta; /* cmd_vel (0,0,0 if none); vy is 0 for a grid      */
  int64_t n_valid;  /* samples with cost >= 0                                */
} sfw_best;

/* 4-double key used for the multi-GPU exchange: lexicographic minimum over
 * ranks reproduces the reference's selection order exactly
 * (cost up, linvel down, |angvel| up, iteration index down). */
typedef struct sfw_best_key {
  double cost;        /* +inf if the rank holds no selectable sample         */
  double neg_linvel;  /* -linvel                                             */
  double abs_angvel;  /* |angvel|                                            */
  double neg_index;   /* -(global iteration index)                           */
} sfw_best_key;

typedef struct sfw_planner_s *sfw_handle;

/* ---- lifecycle --------------------------------------------------------- */
void sfw_params_default(sfw_params *p);
int sfw_abi_version(void);
/* device: HIP device ordinal.  Fails with SFW_ERR_NO_DEVICE when no GPU is
 * visible — there is no CPU fallback in this library. */
int sfw_create(const sfw_params *params, int device, sfw_handle *out);
int sfw_destroy(sfw_handle h);
/* The reference re-reads its parameters on every cycle (:125).
 * Every call that takes parameters — sfw_create, sfw_set_params, sfw_batch_create, sfw_ensemble_create,
 * sfw_ensemble_set_params — answers SFW_ERR_INVALID_ARG, and leaves the handle's parameters as they were, for
 *   - a sim_time or sim_granularity that is not finite, a sim_granularity that is not > 0, a sim_time < 0;
 *   - a step count beyond SFW_MAX_STEPS.  The count is int(sim_time / sim_granularity + 0.5), at least 1 (:519-525); it
 *     is an `int` in every kernel and sizes every table, and a quotient that does not fit an int has no defined
 *     conversion.  What indexes by the count S: the step counters themselves, which run in strides of 8 (S + 8 must
 *     fit); S * K over the footprint's vertices and 3 * S over a pose's components, formed in int; (sample * S + step) * 3,
 *     step * row and chunk * S, formed in 64 bits; and (chunk * S) / 256 blocks of the footprint launch in 32 bits, a
 *     chunk being at least 1024 samples when the stage has as many.  2^20 steps keep every one of the int products
 *     below 2^31 with a factor of 2^10 to spare (1024 footprint vertices) and the block count below 2^32 up to chunks
 *     of 2^20 samples; at the reference's 0.025 s per step they are a horizon of seven hours.  Memory for that many
 *     steps is another matter: a stage that cannot have its tables answers SFW_ERR_HIP;
 *   - max_vel_x that is 0 or not finite: the velocity term is |max_vel_x - vx| / max_vel_x (:654), 0/0 or x/0 there — a
 *     cost that is neither a cost nor a sentinel.  A NEGATIVE max_vel_x is the caller's business: the reference divides
 *     by it unguarded and so does this library (the term is then <= 0).
 * The accelerations of sfw_goal_args must be finite (every stage checks that) and are otherwise the caller's business
 * as well: the reference's computeNewVelocity (:457-463) has a value for a zero and for a negative limit (0: the
 * velocity never changes; negative: min(target, v - |a| dt) runs away from a target above it), and the kernels compute
 * exactly that (tests/test_rollout_gpu.py holds both). */
#define SFW_MAX_STEPS 1048576 /* 2^20 */
int sfw_set_params(sfw_handle h, const sfw_params *params);
const char *sfw_last_error(sfw_handle h);

/* ---- world state (replaces const Costmap2D& / footprint_spec_ / getAgents) */
/* The three calls snapshot their arguments on the host (the caller's buffers may change on return); what has changed
 * reaches the device with the NEXT sfw_grid_stage / sfw_score_* — a launch of a grid staged before the call still
 * scores the old state.
 * cells: row-major, y outer, cells[my*size_x+mx] == Costmap2D::getCost(mx,my) (the reference reads nav2's live
 * costmap, sfw_planner.hpp:362).  A snapshot whose cells and geometry equal the last one's is recognised (a memcmp)
 * and not sent again: hand the live map over every cycle.
 * SFW_ERR_INVALID_ARG: a NULL map, a zero size, a resolution that is not > 0, an origin or resolution that is not finite
 * (a NaN origin would pass every "below the origin" rejection), or a map beyond what the cell arithmetic is good for:
 *   - SFW_MAX_MAP_AXIS_CELLS per axis.  The kernels form a cell index as trunc((w - origin) * (1 / resolution)) and take
 *     the IEEE division the reference executes only when the product lies within 1e-9 of an integer.  Product and
 *     quotient differ by at most 3 * 2^-53 of the quotient (the reciprocal's rounding, the product's, the division's),
 *     so up to a quotient of 1e-9 / (3 * 2^-53) ~ 3.0e6 the two truncations agree whenever the division is not taken;
 *     2^21 cells (and the one cell beyond the border that decides "off the map") stay inside that with a third to spare.
 *   - SFW_MAX_MAP_CELLS in all: the Bresenham walk forms my * size_x + mx in a 32-bit int.
 * 4096 x 4096 cells are far inside both. */
#define SFW_MAX_MAP_AXIS_CELLS 2097152u  /* 2^21 */
#define SFW_MAX_MAP_CELLS 2147483647ull  /* 2^31 - 1 */
int sfw_set_costmap(sfw_handle h, const uint8_t *cells, uint32_t size_x,
                    uint32_t size_y, double origin_x, double origin_y,
                    double resolution);
/* sfw_set_footprint / sfw_set_agents keep a host copy; the next stage
 * (sfw_grid_stage, sfw_score_grid, sfw_score_one) uploads footprint, agents,
 * laser points and the sample vectors in ONE copy.  A sfw_grid_launch without
 * a new stage keeps using what the last stage uploaded. */
/* xy: K points (x0,y0,x1,y1,...) in the robot frame = footprint_spec_
 * (src/sfw_planner.cpp:32).  K < 3 => centre-cell check only
 * (src/costmap_model.cpp:41-48). */
int sfw_set_footprint(sfw_handle h, const double *xy, int32_t K);
/* agents[0] = robot.  obstacles_xy: O laser points shared by every agent's
 * obstacles1 (src/sensor_interface.cpp:513-524).  At most 8190 agents
 * (SFW_ERR_UNSUPPORTED beyond; a set that does not fit one wave's 160 KiB of
 * LDS — roughly 2000 agents — is refused by the scoring call the same way). */
int sfw_set_agents(sfw_handle h, const sfw_agent *agents, int32_t A,
                   const double *obstacles_xy, int32_t O);

/* ---- scoring ----------------------------------------------------------- */
/*
 * The grid loop of findBestAction (src/sfw_planner.cpp:345-417): for every
 * (linvels[iv], angvels[iw]), iv outer, cost = scoreTrajectory(rs, linvel,
 * 0.0, angvel, args...); costs_out[iv*nw+iw] receives it (SFW_COST_SKIPPED
 * for the (0,0) sample).  best_out receives the reference's selection.
 * Blocking: returns after the D2H copy.  costs_out / best_out may be NULL.
 */
int sfw_score_grid(sfw_handle h, const sfw_robot_state *rs,
                   const double *linvels, int32_t nv, const double *angvels,
                   int32_t nw, const sfw_goal_args *args, double *costs_out,
                   sfw_best *best_out);

/*
 * One scoreTrajectory call (the two scalar call sites :204-206, :299-301).
 * points_xyth (nullable) receives up to points_cap (x,y,theta) triples = the
 * Trajectory points (src/sfw_planner.cpp:578); *n_points their count.
 */
int sfw_score_one(sfw_handle h, const sfw_robot_state *rs, double vx_samp,
                  double vy_samp, double vtheta_samp, const sfw_goal_args *args,
                  double *cost_out, double *points_xyth, int32_t points_cap,
                  int32_t *n_points);

/* ---- device-resident pipeline (what sfw_score_grid is made of) --------- */
/* Stage one grid call: one H2D copy of footprint, agents, laser points and
 * the sample vectors; robot state and goal arguments are recorded.  index_base
 * is the global iteration index of this rank's first sample (multi-GPU
 * sharding by linvel rows); 0 on a single GPU. */
int sfw_grid_stage(sfw_handle h, const sfw_robot_state *rs,
                   const double *linvels, int32_t nv, const double *angvels,
                   int32_t nw, const sfw_goal_args *args, int64_t index_base);
/* Enqueue rollout + social-force + argmin kernels on the handle's stream.
 * Everything stays in HBM; no host sync.
 * Stage and launch are all-or-nothing: a call refused for its arguments
 * changes nothing; any other failure leaves nothing staged or launched, so a
 * launch or fetch returns SFW_ERR_STATE until the next successful stage. */
int sfw_grid_launch(sfw_handle h);
int sfw_grid_sync(sfw_handle h);
/* Wait for the launch; the cost vector (nullable) and the local selection (nullable).  Since round 6 the selection kernels
 * themselves leave vector and record in a pinned host buffer of the handle (grids of up to SFW_MIRROR_MAX_MB, default
 * 64 MB, of costs): the call is a wait on the stream — polling it for up to SFW_SPIN_US microseconds, default 20000,
 * before it blocks — plus one memcpy into costs_out; larger grids are copied device-to-host here. */
int sfw_grid_fetch(sfw_handle h, double *costs_out, sfw_best *best_out,
                   sfw_best_key *key_out);
/* The cost vector of the last fetched launch where the handle holds it on the host (nv * nw doubles, sample order;
 * valid until the next sfw_grid_launch / sfw_score_* on this handle), or NULL when this launch was not mirrored (then
 * pass costs_out).  A caller that only reads the vector — a marker publisher, the tests — saves the memcpy:
 * sfw_grid_fetch(h, NULL, &best, NULL) and this. */
const double *sfw_grid_costs_view(sfw_handle h);

/* ---- sample lists ------------------------------------------------------ */
/*
 * Stage a LIST of n samples instead of a grid: sample t is the command
 * (vx[t], vy[t], vtheta[t]).  vy may be NULL: every vy is 0.0.  The list
 * need not be a product of axes: a holonomic (vx, vy, vtheta) window, a set
 * that is denser around the last winner, random or hand-picked candidates.
 * The grid loop's (0,0) skip does not apply: the caller chose the samples.
 *
 * Cost.  costs[t] is bit for bit what the scalar call sfw_score_one returns for
 * (rs, vx[t], vy[t], vtheta[t], args): SFW_COST_INVALID exactly where that
 * call produces it, never SFW_COST_SKIPPED, never NaN.
 *
 * After a list stage sfw_grid_launch / _sync / _fetch / _costs_view /
 * _plan_info, sfw_grid_points(_batch), sfw_set_points_capture,
 * sfw_set_terms_capture, sfw_grid_terms, sfw_grid_rescore, sfw_set_timing and
 * sfw_last_launch_ms act on the list, with sample index t in list order (the
 * cost vector has n entries).  A later sfw_grid_stage replaces the list, a
 * later list stage replaces the grid; the scalar call consumes either.
 * All-or-nothing as for sfw_grid_stage: a call refused for its arguments
 * changes nothing (what was staged before still launches), any other failure
 * leaves nothing staged.
 *
 * SFW_ERR_INVALID_ARG: n < 1; a NULL handle, rs, vx, vtheta or args; a
 * non-finite value in vx, vy, vtheta, rs or args.  SFW_ERR_STATE: no costmap.
 *
 * Selection.  The reference's rule (cost up, linvel down, |angvel| up, later
 * sample first) with linvel = vx[t] and angvel = vtheta[t]; vy takes no part
 * in the order; among equal (cost, vx, |vtheta|) the larger index wins, as in
 * the grid.  sfw_best.index = t and sfw_best.vx / .vy / .vtheta are the
 * sample's own three values (vy is not always 0 here); n_valid counts costs
 * >= 0; sfw_best_key.neg_index = -(index_base + t), so a list can be sharded
 * over ranks as grid rows are.
 *
 * sfw_plan_info of a list: samples = n; levels = split_step = classes =
 * class_steps = 0 — there is NO shared-prefix rollout for lists: a list has
 * no axes along which samples share their first steps, so every sample is
 * integrated over the whole horizon.  Where the samples ARE a product of two
 * axes keep using sfw_grid_stage: at the target configuration (256 x 256
 * samples, 20 people) the grid's shared prefix integrates about 73 % of the
 * sample-steps the list does (how much slower the list is there has not been
 * measured yet, see CHANGELOG.md; examples/sample_list_latency.cpp prints the
 * ratio).  organisation, chunks and flat_samples are those of
 * a grid of n x 1; one_launch is 1 exactly where a grid of the same size and
 * crowd gets it (a refinement list of a few dozen samples is ONE kernel
 * launch); rest_noise_unreproduced looks at the list's samples as it looks at
 * a grid's rows (a sample with vx == 0 and vy == 0).
 *
 * A member of a sfw_batch may be staged with a list: its results after
 * sfw_batch_launch / _fetch are bit-identical to its own launch.  By default
 * it does not join the batched kernel (sfw_batch_desc.own_path_members counts
 * it); with sfw_batch_set_list_fusion(b, 1) a list whose launch is the
 * one-kernel cycle (one_launch) joins the batched launch of the lists
 * (one_launch_members).  sfw_batch_score_samples scores one list per member;
 * sfw_multi_* take grids only; an ensemble scores a list as sequences of one
 * knot (sfw_ensemble_score_sequences, K == 1).
 */
int sfw_samples_stage(sfw_handle h, const sfw_robot_state *rs, const double *vx, const double *vy,
                      const double *vtheta, int32_t n, const sfw_goal_args *args, int64_t index_base);
/* sfw_samples_stage (index_base 0) + sfw_grid_launch + sfw_grid_fetch: costs_out (nullable) receives n costs. */
int sfw_score_samples(sfw_handle h, const sfw_robot_state *rs, const double *vx, const double *vy,
                      const double *vtheta, int32_t n, const sfw_goal_args *args, double *costs_out,
                      sfw_best *best_out);

/* Command SEQUENCES: samples whose command changes inside the horizon
 * ("brake for 0.3 s, then swing left", last cycle's plan with a varied tail,
 * the rollouts of a sampling MPC / MPPI controller).  A sample is K knots;
 * vx, vy (nullable: all 0.0) and vtheta hold K x n doubles, KNOT-major: knot
 * k of sample t at [k * n + t].  knot_step[K] is shared by all samples:
 * knot_step[0] == 0, strictly ascending.  At Euler step i the three targets
 * of computeNewVelocity are those of knot k(i), the largest k with
 * knot_step[k] <= i.  Everything else is the reference's scoreTrajectory
 * statement by statement: the acceleration clip runs from the running
 * velocity every step, Euler integrates with the old heading, the velocity
 * term reads the last step's vx, distance and angle come from the final
 * pose, costmap mean, pedestrian contact and social work as in the
 * reference.  A knot whose step is >= the step count is never reached and is
 * no error (sfw_set_params may change the step count between stage and
 * launch; the knots are looked up by the kernels as the steps go by).
 *
 * Contract (tests/test_sequences_gpu.py holds each point):
 *  1. K == 1 is sfw_samples_stage: costs, sentinels, selection, terms, points
 *     and crowd are bit-identical (the list's kernels run).
 *  2. A sequence whose knots all carry the same command has bit for bit the
 *     cost of that command in a list, whatever knot_step is.
 *  3. Cutting the knots at the horizon changes nothing: the knots at steps
 *     >= S may be removed.
 *  4. Causality: two samples whose knots agree up to the knot active at step
 *     j have bit-identical Trajectory points 0..j+1 and crowd rows 0..j.
 *  5. A sample's result does not depend on where it stands in the stage or
 *     what stands beside it, on whether the one-launch kernel scored it
 *     (SFW_CYCLE_FUSED), on how the stage is chunked (SFW_TABLE_BUDGET_MB), or
 *     on which pose-rollout kernel walked it.
 *  6. Costs are never SFW_COST_SKIPPED and never NaN; SFW_COST_INVALID
 *     appears exactly where the reference would return -1.0.
 *
 * Selection: the reference's rule with linvel = vx[0 * n + t] and angvel =
 * vtheta[0 * n + t] — the FIRST knot is the command the controller sends
 * now.  sfw_best.vx / .vy / .vtheta are the winner's first knot, index = t,
 * sfw_best_key.neg_index = -(index_base + t).
 *
 * After a sequence stage everything that acts on a staged list acts on the
 * sequences in sample order: sfw_grid_launch / _sync / _fetch / _costs_view /
 * _plan_info, sfw_grid_points(_batch), sfw_set_points_capture,
 * sfw_set_terms_capture, sfw_grid_terms, sfw_grid_rescore, sfw_grid_crowd,
 * sfw_set_timing, sfw_last_launch_ms.  Grid, list and sequence stages replace
 * one another; sfw_score_one consumes any of them.  All-or-nothing as for
 * every stage: a call refused for its arguments changes nothing, any other
 * failure leaves nothing staged.
 *
 * SFW_ERR_INVALID_ARG (before any device call): n < 1; K < 1 or K >
 * SFW_SEQ_MAX_KNOTS; a NULL h, rs, vx, vtheta, knot_step or args;
 * knot_step[0] != 0 or knot_step not strictly ascending; a non-finite value
 * in any knot, in rs or in args.  SFW_ERR_STATE: no costmap.
 *
 * sfw_plan_info reports what a list reports (no shared prefix, one_launch
 * under the list's conditions).  rest_noise_unreproduced is set when a person
 * is pinned (desired_velocity == 0), there are at least two agents, and for
 * some sample the velocity recurrence over its knots REACHES translation
 * velocity (0, 0) after a step i < S - 1 having been non-zero at hand-over or
 * after an earlier step.  A robot that stands from hand-over and starts to
 * move at a later knot is at rest at the handed-over pose only: reproduced,
 * flag 0.
 *
 * A member of a sfw_batch may be staged with sequences: by default it takes
 * its own path (sfw_batch_desc.own_path_members); with
 * sfw_batch_set_list_fusion(b, 1) sequences whose launch is the one-kernel
 * cycle join the batched launch of the sequences (K == 1: of the lists).
 * Either way bit-identical to its own launch.  sfw_batch_score_sequences /
 * _score_perturbed score one set of sequences per member; sfw_multi_* keep
 * taking grids only; an ensemble scores sequences through
 * sfw_ensemble_score_sequences / _score_perturbed.
 */
#define SFW_SEQ_MAX_KNOTS 64
int sfw_sequences_stage(sfw_handle h, const sfw_robot_state *rs, const double *vx, const double *vy,
                        const double *vtheta, int32_t n, int32_t K, const int32_t *knot_step,
                        const sfw_goal_args *args, int64_t index_base);
/* sfw_sequences_stage (index_base 0) + sfw_grid_launch + sfw_grid_fetch: costs_out (nullable) receives n costs. */
int sfw_score_sequences(sfw_handle h, const sfw_robot_state *rs, const double *vx, const double *vy,
                        const double *vtheta, int32_t n, int32_t K, const int32_t *knot_step,
                        const sfw_goal_args *args, double *costs_out, sfw_best *best_out);

/* PERTURBED sequences: the rollouts of a sampling controller (MPPI) drawn on
 * the device.  sfw_sequences_perturb_stage is sfw_sequences_stage whose K x n
 * knots are not handed over but computed by a kernel from a nominal plan of K
 * knots, a standard deviation and a clamp box per channel, and a seed: under
 * 2 KB go to the device instead of 24 K n bytes.
 *
 * Definition.  For sample t, knot k and channel c (0 vx, 1 vy, 2 vtheta), with
 * g = index_base + t as an unsigned 64-bit number:
 *   (w0, w1, w2, w3) = Philox4x32-10(counter = (g & 0xffffffff, g >> 32, k, c),
 *                                    key = (seed & 0xffffffff, seed >> 32))
 *     — the Random123 generator: multipliers 0xD2511F53 and 0xCD9E8D57, Weyl
 *     constants 0x9E3779B9 and 0xBB67AE85, ten rounds;
 *   m1 = ((w1 << 32) | w0) >> 11,  u1 = (m1 + 1) * 2^-53   in (0, 1];
 *   m2 = ((w3 << 32) | w2) >> 11,  u2 = m2 * 2^-53         in [0, 1);
 *   r = sqrt(-2.0 * log(u1)),  z = r * cos(6.283185307179586 * u2)
 *     — the argument of cos is one IEEE product; log and cos are the device
 *     library's double functions (as the blend's exp is), sqrt is IEEE; the
 *     sine branch of Box-Muller is discarded;
 *   under SFW_PERTURB_KEEP_NOMINAL z = 0.0 where g == 0;
 *   u = fmin(fmax(nominal[k][c] + sigma[c] * z, lo[c]), hi[c])
 *     — the product and the sum are each rounded on their own (no
 *     contraction).
 * social_force_window_planner_amd/perturb.py restates this in numpy
 * (perturb.reference); tests/test_perturb_gpu.py holds the device to it.
 *
 * Consequences.  r <= sqrt(106 ln 2) < 8.58, so every knot is finite.  A
 * value depends on (seed, g, k, c, nominal[k][c], sigma[c], lo[c], hi[c]) and
 * on nothing else: not on n, not on K beyond k, not on the neighbouring
 * samples, not on SFW_DEVICE_CUS, SFW_TABLE_BUDGET_MB or SFW_CYCLE_FUSED, and
 * not on how a list is sharded over ranks — shards that pass their index_base
 * draw what the unsharded stage draws.  The same seed draws the same
 * perturbations: the caller changes `seed` from cycle to cycle.
 *
 * Under SFW_PERTURB_NO_VY the stage has no vy vector (vy == NULL in
 * sfw_sequences_stage): channel 1 of every knot is 0.0 whatever the box says.
 *
 * The stage is a sequence stage in every respect: sfw_grid_launch / _sync /
 * _fetch / _costs_view / _plan_info, sfw_grid_points(_batch), the terms and
 * points capture, sfw_grid_rescore, sfw_grid_crowd, sfw_grid_blend, timing and
 * a batch member's own path act on it as on sfw_sequences_stage, and a second
 * stage by sfw_sequences_stage with the knots sfw_sequences_knots returns is
 * BIT FOR BIT the perturbed stage in everything it produces.  K == 1 runs the
 * list's kernels.  sfw_best.vx / .vy / .vtheta are bitwise the winner's first
 * knot as sfw_sequences_knots reports it (one small copy from the device
 * behind the fetch's wait: the host never holds the knots).
 *
 * rest_noise_unreproduced of a perturbed stage is CONSERVATIVE, because the
 * host never sees the knots: 1 when a person is pinned, there are at least two
 * agents and the clamp box admits a zero translation command — lo[0] <= 0 <=
 * hi[0] and (SFW_PERTURB_NO_VY or lo[1] <= 0 <= hi[1]) — else 0.
 *
 * SFW_ERR_INVALID_ARG (before any device call; a refused call changes
 * nothing): a NULL h, rs, p, p->nominal, knot_step or args; n < 1; K outside
 * [1, SFW_SEQ_MAX_KNOTS]; knot_step[0] != 0 or not strictly ascending;
 * index_base < 0; a non-finite value in nominal, sigma, lo, hi, rs or args;
 * sigma[c] < 0; lo[c] > hi[c]; unknown flag bits or reserved != 0;
 * SFW_PERTURB_NO_VY with sigma[1] != 0 or some nominal[k][1] != 0.
 * SFW_ERR_STATE: no costmap.  All-or-nothing as every stage is.
 */
#define SFW_PERTURB_KEEP_NOMINAL 1  /* the sample with GLOBAL index index_base + t == 0 gets z = 0 in every channel */
#define SFW_PERTURB_NO_VY        2  /* stage without a vy vector, as vy == NULL in sfw_sequences_stage */
#define SFW_PERTURB_KEEP_NORMALS 4  /* also keep every z on the device for sfw_sequences_normals */
typedef struct sfw_perturb {
  uint64_t seed;
  const double *nominal;  /* K x 3 doubles: [k][vx, vy, vtheta] */
  double sigma[3];        /* per channel, finite, >= 0 */
  double lo[3], hi[3];    /* clamp box per channel, finite, lo <= hi */
  int32_t flags, reserved;
} sfw_perturb;
int sfw_sequences_perturb_stage(sfw_handle h, const sfw_robot_state *rs, const sfw_perturb *p, int32_t n, int32_t K,
                                const int32_t *knot_step, const sfw_goal_args *args, int64_t index_base);
/* sfw_sequences_perturb_stage (index_base 0) + sfw_grid_launch + sfw_grid_fetch: costs_out (nullable) receives n costs. */
int sfw_score_perturbed(sfw_handle h, const sfw_robot_state *rs, const sfw_perturb *p, int32_t n, int32_t K,
                        const int32_t *knot_step, const sfw_goal_args *args, double *costs_out, sfw_best *best_out);
/* The knots of samples [first, first + count) of the staged list or sequences (host-staged or perturbed), knot-major within
 * the range: out[k * count + i] is knot k of sample first + i.  vy_out is nullable; a stage without a vy vector reports 0.0.
 * SFW_ERR_STATE: nothing staged, or a grid.  SFW_ERR_INVALID_ARG: a range outside [0, n), count < 1, a NULL vx_out or
 * vtheta_out. */
int sfw_sequences_knots(sfw_handle h, int64_t first, int64_t count, double *vx_out, double *vy_out, double *vtheta_out);
/* The normals z of the same range of a perturbed stage: z_out[(k * 3 + c) * count + i] (all three channels, whatever
 * SFW_PERTURB_NO_VY says).  SFW_ERR_STATE unless the stage was perturbed with SFW_PERTURB_KEEP_NORMALS. */
int sfw_sequences_normals(sfw_handle h, int64_t first, int64_t count, double *z_out);

/* How the staged grid will be launched.  levels > 0: the shared-prefix
 * rollout is in use — under the acceleration limits (sfw_planner.hpp:457-463)
 * the robot's first steps are bit-identical for all samples of a class (same
 * clipped linear x angular velocity sequences; the angular one a step shorter,
 * see sfw_plan_shared_prefix_items), and classes refine step by
 * step, so the first split_step steps are simulated along a tree of `levels`
 * levels of classes (class_steps class-steps in all instead of
 * samples * split_step sample-steps) and every sample resumes from its class
 * of the last level (`classes` of them).  Costs are bit-identical to the
 * plain rollout; SFW_PREFIX=0 in the environment of sfw_create switches it
 * off, SFW_PREFIX=3,7,12 forces the levels' end steps. */
#define SFW_ORG_NONE 0       /* no agents: the social-force kernel is not launched             */
#define SFW_ORG_REGISTER_1 1 /* register-resident, one agent slot per lane (A <= 64, floor(64/A) samples per wave) */
#define SFW_ORG_REGISTER_2 2 /* register-resident, two agent slots per lane (64 < A <= 128)      */
#define SFW_ORG_FLAT 3       /* all unordered pairs flattened over the lanes, one sample per wave */
typedef struct sfw_plan_info {
  int32_t split_step;  /* last shared step + 1; 0: plain rollout             */
  int32_t levels;
  int32_t chunks;      /* launches of the K1->K2 table (SFW_TABLE_BUDGET_MB) */
  int32_t organisation; /* SFW_ORG_*: how a wave of the launch over the SAMPLES is organised (the suffix
                           launch of the shared-prefix rollout, or the whole rollout); the prefix levels
                           pick theirs by their class counts.  Costs do not depend on it.  */
  int64_t classes;     /* work items of the last level (sfw_plan_shared_prefix_items), summed over chunks */
  int64_t class_steps; /* sum over levels of items x steps of the level      */
  int64_t samples;     /* nv * nw                                            */
  int64_t flat_samples; /* organisation = SFW_ORG_REGISTER_1 only: samples (of the first chunk's launch) that the launch
                           hands to flat-form waves running beside the register-form ones, so that every SIMD holds
                           the same number of those (0: none).  Costs do not depend on it.                      */
  int64_t one_launch;   /* 1: a control cycle's grid (<= 1024 samples, fewer than 64 agents, flat form) — rollout,
                           footprint checks, pedestrian simulation and selection run as ONE kernel launch.  Costs,
                           sentinels and selection do not depend on it (SFW_CYCLE_FUSED=0 in the environment: never). */
  int64_t rest_noise_unreproduced; /* 1: this stage holds the one configuration whose reference result is NOT reproduced
                           (see sfw_agent.desired_velocity): a person that can never move (desired_velocity == 0) AND a
                           robot that moves now but BRAKES TO A STOP inside the rollout of some sample (a linvel sample of
                           0 whose deceleration ends before the horizon).  From the step the robot stands, the pair is at
                           exact relative rest at a position the device's own pose rollout produced; lightsfm's lateral
                           term there is the rounding noise of two atan2 on the host's libm (0 for most geometries, a
                           full-magnitude +-1 for the others) and the kernels' is 0.  Affects those samples' social work
                           only; 0 for every other stage, incl. the robot that stands still from the start (reproduced). */
} sfw_plan_info;
int sfw_grid_plan_info(sfw_handle h, sfw_plan_info *out);
/* The plan a single-chunk stage of this grid would choose ON A WHOLE MI355X
 * (256 compute units; SFW_DEVICE_CUS in the environment pretends another
 * count, as it does for a handle — a handle on a partition reads its own
 * device and may plan differently: sfw_grid_plan_info says what it chose),
 * computed on the host alone (no handle, no device): end steps of the levels and their class
 * counts (row classes x column classes), up to cap entries; *n_levels = 0
 * when sharing does not pay (fewer than 4096 samples, fewer than two agents,
 * or nothing to share).  vx0 / vtheta0: the robot's current velocities,
 * acc_*: sfw_goal_args, num_steps as scoreTrajectory derives it (:519-525). */
int sfw_plan_shared_prefix(const double *linvels, int32_t nv,
                           const double *angvels, int32_t nw, double vx0,
                           double vtheta0, double acc_x, double acc_theta,
                           double sim_time, int32_t num_steps,
                           int32_t n_agents, int32_t *level_ends,
                           int64_t *level_classes, int32_t cap,
                           int32_t *n_levels);
/* The WORK ITEMS of the same plan (same arguments, same level_ends): what a level's launch integrates once each.  A level
 * ending at step p reads the robot's records of steps 0..p-1 only, and a record holds the position after its step, which takes
 * the heading BEFORE the step (sfw_planner.cpp:586-588): records 0..p-1 depend on the linear velocities of steps 0..p-1 but on
 * the angular velocities of steps 0..p-2.  So the items of the level are row classes(p) x column classes(p - 1) — one column
 * class for p = 1 —, fewer than the velocity classes sfw_plan_shared_prefix reports (row classes(p) x column classes(p): the
 * samples whose first p commanded velocities coincide).  sfw_plan_info.classes / class_steps count items. */
int sfw_plan_shared_prefix_items(const double *linvels, int32_t nv, const double *angvels, int32_t nw, double vx0,
                                 double vtheta0, double acc_x, double acc_theta, double sim_time, int32_t num_steps,
                                 int32_t n_agents, int32_t *level_ends, int64_t *level_items, int32_t cap, int32_t *n_levels);
/* One axis of that plan (host only; diagnostics and tests): the classes of `n` target velocities whose first p clipped
 * velocities (computeNewVelocity, sfw_planner.hpp:457-463, from the current velocity v0 under a_max, dt) are bit-equal,
 * for p = 1 .. *n_levels <= max_p (the walk stops once every target is its own class).  counts[p-1] = classes of level
 * p; classes (nullable) receives [level][n] class ids, numbered in target order.  form 0: the planner's own choice (the
 * closed form over the two "not yet reached" groups where its premises hold — *closed_form says so —, else the generic
 * walk of every target's recurrence); form 1: the generic walk.  Both give the same classes. */
int sfw_plan_axis_classes(const double *targets, int32_t n, double v0, double a_max, double dt, int32_t max_p,
                          int32_t form, int32_t *counts, int32_t *classes, int32_t *n_levels, int32_t *closed_form);
/* Contiguous blocks of linvel rows of about equal PLANNED work for R ranks (host only): row0[0..R], rank r takes rows
 * [row0[r], row0[r+1]).  The share of steps the shared-prefix tree saves differs along the row axis (BASELINE cfg5 cut
 * into 8 equal blocks integrates 64..76 % of its steps per block), so equal row counts are unequal work; the cuts follow
 * the planned class-steps instead.  Equal row counts when nothing is shared (fewer than 4096 samples per rank, fewer
 * than two agents).  sfw_multi_score_grid cuts this way; multi-process callers use it to agree on the same cut. */
int sfw_plan_row_blocks(const double *linvels, int32_t nv, const double *angvels, int32_t nw, double vx0,
                        double vtheta0, double acc_x, double acc_theta, double sim_time, int32_t num_steps,
                        int32_t n_agents, int32_t R, int32_t *row0);
/* Tuning / test knob: which organisation the social-force kernel's waves use.  SFW_K2_AUTO (default) picks
 * per launch by agent and item count; SFW_K2_REGISTER / SFW_K2_FLAT force one wherever it exists for the
 * agent count (register: A <= 128; flat: A >= 2, or laser points).  The organisations are bit-identical in
 * their results.  Takes effect at the next stage.  SFW_FORCE_FLAT=0|1 in the environment of sfw_create sets
 * the handle's initial value. */
#define SFW_K2_AUTO (-1)
#define SFW_K2_REGISTER 0
#define SFW_K2_FLAT 1
int sfw_set_k2_form(sfw_handle h, int32_t form);
/* Per-kernel HIP events around the kernels of sfw_grid_launch, off by default
 * (a control cycle is latency-bound; four event records cost as much as a
 * kernel).  Measurement tooling (bench.py) switches them on. */
int sfw_set_timing(sfw_handle h, int32_t enabled);
/* HIP-event time (ms) of the most recent sfw_grid_launch (SFW_ERR_STATE unless
 * timing was on): which = 0 whole launch, 1 rollout kernels, 2 social-force
 * kernel, 3 argmin. */
int sfw_last_launch_ms(sfw_handle h, int32_t which, float *ms_out);
/* Shader clock (GHz) the social-force kernel of the most recent timed sfw_grid_launch really ran at: the middle wave of the
 * launch over the samples reads the core-clock and the constant-rate counters when it starts and when it ends.
 * 0.0 when there was nothing to sample (no agents).  Boxes and thermal states differ by ~10 %: a kernel time is
 * only comparable across runs next to this number.  SFW_ERR_STATE unless timing was on. */
int sfw_last_clock_ghz(sfw_handle h, double *ghz_out);
/* Optional dump of the per-step robot poses of sample `index` of the last
 * launch (Trajectory points for RViz markers, :366-374). */
int sfw_grid_points(sfw_handle h, int64_t index, double *points_xyth,
                    int32_t points_cap, int32_t *n_points);
/* The same for `count` consecutive samples starting at `first` in one call (the
 * reference fills one RViz marker per sample every cycle, :347-386).
 * points_xyth: count x steps x 3 doubles (steps = num_steps of the params),
 * n_points: count ints = poses the reference's Trajectory would hold: all of them
 * for a valid sample, those before the first illegal footprint pose, or 0..i for a
 * sample rejected by pedestrian contact at step i (0 for the (0,0) sample).
 * A sample that is illegal on the costmap at pose j AND touches a pedestrian at an earlier step i < j
 * reports i + 1 poses, as the reference does (it returns at the contact, :613-627): when the range holds
 * costmap-rejected samples their pedestrians are integrated in an extra pass of this call. */
int sfw_grid_points_batch(sfw_handle h, int64_t first, int64_t count, double *points_xyth, int32_t *n_points);
/* Marker support without a second rollout: with capture on, a scoring launch over a grid small enough for the
 * one-launch rollout (at most 2048 samples and 512 steps: a control cycle's 5 x 9 samples) also leaves every
 * sample's Trajectory points, point count and contact step on the device, and sfw_grid_points(_batch) of that
 * launch is ONE device-to-host copy instead of re-running the rollout (and, when a sample was rejected on the
 * costmap, the pedestrian integration).  Costs and selection are unaffected.  Larger grids ignore it.  Off by
 * default; takes effect at the next sfw_grid_launch / sfw_score_grid. */
int sfw_set_points_capture(sfw_handle h, int32_t enabled);
/* The footprint check's clearance map, on by default.  One byte per costmap cell on the device: 1 where every cell of
 * the square window of half-width r_c = ceil(R / resolution) + 1 cells (R: the largest vertex distance of the
 * footprint) around the cell is on the map and has cost 0.  A pose whose centre cell is clear has footprint cost 0
 * whatever its heading, and the check returns it without converting a vertex or walking an edge; every other pose is
 * checked as before.  Costs, sentinels, selection, captured terms and points are bit-identical on and off.
 * The map is built by the first stage (sfw_grid_stage, sfw_samples_stage, sfw_sequences_*_stage and the blocking calls
 * over them) of at least 368 640 poses (samples x steps: 96 x 96 samples at 40 steps) after the costmap's contents or size, or the window's
 * half-width (footprint, resolution), have changed — two small kernels on the handle's stream behind the upload of the
 * cells, about as long as the upload itself — and kept until they change again; smaller grids (a control cycle) never
 * pay for it and walk every pose.  No map either when the window would be wider than 129 cells.  Off: no stage builds or
 * reads a map; takes effect at the next launch (turned on again, at the next stage). */
int sfw_set_footprint_clearance(sfw_handle h, int32_t on);
/* Of the staged grid: *built = 1 when its footprint checks read a clearance map, *half_width = r_c in cells (-1: the
 * footprint is too large for a map).  SFW_ERR_STATE when nothing is staged. */
int sfw_footprint_clearance_info(sfw_handle h, int32_t *built, int32_t *half_width);
/* The staged grid's clearance map, size_x * size_y bytes, row-major like the costmap (tests and inspection; blocking).
 * SFW_ERR_STATE when the staged grid has none, SFW_ERR_INVALID_ARG when cells is not size_x * size_y. */
int sfw_footprint_clearance_map(sfw_handle h, uint8_t *out, uint64_t cells);
/* Raw HIP stream (hipStream_t) the handle launches on, for callers that want
 * to record their own events. */
void *sfw_stream(sfw_handle h);

/* ---- per-term costs and re-scoring under other weights --------------------
 * A sample's cost is the sum of five weighted terms (src/sfw_planner.cpp:643-667; the reference's debug line prints them,
 * :668-674), and the weights are the only part of sfw_params that enters after the rollout: validity (off-map poses,
 * illegal footprints, pedestrian contact) never depends on them.  With capture on, a scoring launch keeps the five
 * unweighted terms of every sample, and any weight vector can be applied to them again without another rollout — the
 * per-critic breakdown of a nav2 controller, or "what would the planner pick under these weights?". */
#define SFW_TERM_VEL 0      /* vel_diff = |max_vel_x - vx| / max_vel_x (:654)                                */
#define SFW_TERM_DISTANCE 1 /* d = squared distance from the final pose to the way-point (:643-646)        */
#define SFW_TERM_ANGLE 2    /* ang_diff = |normalizeAngle(atan2 - theta)| / pi (:647-652)                  */
#define SFW_TERM_COSTMAP 3  /* costmap_cost = mean footprint cost / 255 over the steps (:575, :656)        */
#define SFW_TERM_SOCIAL 4   /* social_work of the pedestrian simulation (:613-629); 0.0 without agents    */
#define SFW_N_TERMS 5
#define SFW_RESCORE_MAX_K 1024
/* One weight vector = the five weights of sfw_params in term order. */
typedef struct sfw_weights {
  double vel, distance, angle, costmap, social; /* vel_weight, distance_weight, angle_weight, costmap_weight, social_weight */
} sfw_weights;
/* Term capture, off by default; takes effect at the next sfw_grid_launch / sfw_score_grid (also in a sfw_batch_launch:
 * batch members carry the capture buffer in their record of the batched cycle kernel — no member changes path for it).
 * Every grid launch then also writes the five terms of every sample into a device buffer of the handle, SoA [5][nv*nw],
 * from the same statements that form the cost: 40 bytes per sample (2.6 MB at 256 x 256 samples, 671 MB at 4096 x 4096),
 * allocated by the first stage or launch that captures, grown with the grid, freed when capture is turned off (after a wait
 * for the handle's stream) or the handle is destroyed.  A sample whose cost is a sentinel (SFW_COST_INVALID, SFW_COST_SKIPPED) has
 * that sentinel in all five terms.  Costs, sentinels, selection and captured points do not depend on it. */
int sfw_set_terms_capture(sfw_handle h, int32_t enabled);
/* K weight vectors (1 <= K <= SFW_RESCORE_MAX_K, all finite: else SFW_ERR_INVALID_ARG) over the terms of the handle's last
 * launch: best_out (K records) receives for every k what sfw_score_grid would return with those five weights in sfw_params —
 * field for field, incl. n_valid (a negative weight can make a cost negative, hence unselectable, as in the reference), the
 * cost == 10000.0 rule, the tie-breaks and index_base; costs_out (nullable) K x nv*nw doubles, weight-major, sample order,
 * bit-identical to that call's cost vector.  One kernel over samples x weight tiles plus a K-way reduction on the handle's
 * stream, ordered behind the launch; blocking.  Read-only for the launch: its cost vector (sfw_grid_costs_view,
 * sfw_grid_fetch), selection and captured points stay as they were.  SFW_ERR_STATE when the last launch did not capture
 * terms, or a stage or sfw_score_one came in since. */
int sfw_grid_rescore(sfw_handle h, const sfw_weights *w, int32_t K, sfw_best *best_out, double *costs_out);
/* count x 5 doubles, sample-major (terms_out[i * 5 + k] = term k of sample first + i), of the last launch; valid under the
 * same conditions as sfw_grid_rescore.  One device-to-host copy per term. */
int sfw_grid_terms(sfw_handle h, int64_t first, int64_t count, double *terms_out);

/* ---- softmin blend: the update of a sampling controller (MPPI) ---------------
 * A sampling controller does not want the argmin of its n rollouts' costs; it wants their softmin weights, the normaliser
 * and effective sample size, and the weighted mean of the command knots — its next nominal plan.  Costs and knots are on the
 * device after a launch; this call reduces them there, for L temperatures at once, and returns a few hundred bytes.
 *
 * It acts on the handle's last launch, whatever was staged.  T = samples, K = knots per sample: a grid has K = 1 and sample
 * t = iv*nw+iw the command (linvels[iv], 0.0, angvels[iw]); a list has K = 1; sequences have their K knots.
 *   valid_t    cost_t >= 0 (the set sfw_best.n_valid counts; sentinels and negative costs are not valid)
 *   J_t        cost_t + bias_t, one IEEE addition (bias == NULL: cost_t itself).  bias (nullable, T doubles) carries the
 *              caller's control-cost term lambda * u^T Sigma^-1 eps, or any per-sample prior; at an invalid sample it is ignored
 *   j_min      the minimum of J over the valid samples; index_min the LARGEST t that holds it (the selection's tie-break);
 *              j_min = J[index_min]
 *   a_t        (J_t - j_min) / lambda_l: one IEEE subtraction, one IEEE division
 *   w_t        exp(-a_t), the device library's double exp; exactly 0.0 at an invalid sample.  The samples at j_min have
 *              w == 1.0 exactly, a_t = +inf gives exactly 0.0
 *   eta        sum_t w_t;   sum_w2 = sum_t (w_t * w_t);   effective sample size = eta * eta / sum_w2
 *   u_out      [l][k][vx, vy, vtheta] = (sum_t w_t * u[k][t]) / eta: every product rounded on its own (no contraction), one
 *              division at the end.  The vy channel of a grid, or of a stage without vy, is 0.0
 *   weights_out (nullable) L x T doubles, lambda-major.
 * No valid sample: every stat_out[l] = {lambda_l, j_min -1.0, eta 0.0, sum_w2 0.0, n_valid 0, index_min -1}, every entry of
 * u_out 0.0, every weight 0.0, SFW_OK.  j_min, n_valid and index_min do not depend on l.
 *
 * Determinism.  eta, sum_w2 and every u channel are sums of T terms x_t (w_t, w_t * w_t, w_t * u[k][t]; an invalid sample's
 * term is its product with w_t = 0.0).  Each goes through ONE summation tree that is a function of T alone — not of the
 * device's compute units (SFW_DEVICE_CUS), of how the scoring launch was chunked (SFW_TABLE_BUDGET_MB), of whether the
 * one-launch kernel scored the stage (SFW_CYCLE_FUSED), of L, or of whether weights_out was asked for.  With C = 256,
 * B = ceil(T / C) and x_t = +0.0 for T <= t < B * C:
 *   1. wave:   block b owns samples [b*C, (b+1)*C); lane i of wave v of the block holds x at t = b*C + 64*v + i.  Butterfly:
 *              for d = 32, 16, 8, 4, 2, 1 in that order every lane replaces its value by (its own + lane (i xor d)'s).
 *              After the six levels every lane holds the wave's sum s_v.
 *   2. block:  p_b = ((s_0 + s_1) + s_2) + s_3.
 *   3. blocks: sum = (...((p_0 + p_1) + p_2) ... ) + p_(B-1), in block order.
 * Every + is one IEEE double addition; no floating-point atomics.  A term passes through d(T) = 6 + 3 + (B - 1) additions at
 * most (the depth of the tree).  social_force_window_planner_amd/blend.py restates definition and tree in numpy
 * (blend.reference, blend.depth); tests/test_blend_gpu.py holds the device to it bit for bit.
 *
 * State: read-only for the launch, as sfw_grid_rescore — the cost vector, selection, captured points and terms and
 * sfw_grid_crowd stay valid; needs no terms capture; works on a batch member after sfw_batch_fetch.  SFW_ERR_STATE when
 * there is no launch, or a stage or sfw_score_one came in since.  Three small kernels on the handle's stream behind the
 * launch; blocking.
 * SFW_ERR_INVALID_ARG (before any device call; a refused call changes nothing): a NULL h, lambda, stat_out or u_out; L
 * outside [1, SFW_BLEND_MAX_L]; a lambda that is not finite or not > 0; a non-finite bias value. */
#define SFW_BLEND_MAX_L 16
typedef struct sfw_blend_stat {
  double lambda;      /* the temperature this record belongs to                          */
  double j_min;       /* min over valid samples of J_t; -1.0 when there is none          */
  double eta;         /* sum of w_t                                                      */
  double sum_w2;      /* sum of w_t * w_t  (effective sample size = eta * eta / sum_w2)  */
  int64_t n_valid;    /* samples with cost >= 0: sfw_best.n_valid of the same launch     */
  int64_t index_min;  /* the LARGEST t with J_t == j_min (the selection's tie-break); -1 */
} sfw_blend_stat;
int sfw_grid_blend(sfw_handle h, const double *lambda, int32_t L, const double *bias,
                   sfw_blend_stat *stat_out, double *u_out, double *weights_out);

/* ---- MPPI on the device: the control cost, and chained iterations ------------
 * Control cost.  MPPI's importance weight carries u_nom^T Sigma^-1 eps_t, the control-cost term of sample t's perturbation.
 * After sfw_sequences_perturb_stage the host holds no perturbations; these calls form the term on the device from what the
 * stage was drawn from.  For sample t of the staged PERTURBED sequences, z[k][c] is bit for bit the normal of the stage's
 * Definition (the value sfw_sequences_normals reports; 0.0 at g == 0 under SFW_PERTURB_KEEP_NOMINAL):
 *   acc = +0.0
 *   for k = 0 .. K-1:  for c = 0, 1, 2 with sigma[c] > 0:
 *       q   = nominal[k][c] / sigma[c]      one IEEE division
 *       acc = acc + q * z[k][c]             product and sum each rounded on their own (no contraction)
 *   c_t = acc;   bias_t = gamma * c_t       one IEEE product
 * A channel with sigma[c] == 0 is skipped (under SFW_PERTURB_NO_VY channel 1 always is: its sigma is 0).  This is
 * u_nom^T Sigma^-1 eps_t with the UNCLAMPED eps = sigma * z.  The value depends on (seed, g, K, nominal, sigma, flags) alone:
 * not on SFW_PERTURB_KEEP_NORMALS (the kept normals are read where the stage kept them, else drawn again: the same bits),
 * not on n, on chunking, on SFW_DEVICE_CUS or on SFW_CYCLE_FUSED.  social_force_window_planner_amd/mppi.py restates it in
 * numpy (mppi.control_cost); tests/test_mppi_gpu.py holds the device to it bit for bit.
 *
 * sfw_sequences_control_cost: bias_out[t] = gamma * c_t, n doubles.  One kernel and one copy on the handle's stream; blocking.
 * It needs a valid perturbed stage (sfw_sequences_perturb_stage, sfw_score_perturbed, sfw_mppi_run), before or after its
 * launch, and leaves stage and launch as they are.  SFW_ERR_STATE: nothing staged, a grid, a host-staged list or sequences.
 * SFW_ERR_INVALID_ARG (before any device call): a NULL h or bias_out, a gamma that is not finite.
 *
 * sfw_grid_blend_control: sfw_grid_blend with J_t = cost_t + b_t, where b_t = gamma * c_t (bias == NULL) or
 * (gamma * c_t) + bias_t, each + one IEEE addition; nothing else differs — the definition, the outputs, the summation tree
 * and the state rule are sfw_grid_blend's.  The bias vector never leaves the device.  gamma == 0 is bit for bit
 * sfw_grid_blend with the same `bias`.  SFW_ERR_STATE: as sfw_sequences_control_cost, and sfw_grid_blend's own rule (no
 * launch).  SFW_ERR_INVALID_ARG (before any device call; a refused call changes nothing): what sfw_grid_blend refuses, and
 * a gamma that is not finite. */
int sfw_sequences_control_cost(sfw_handle h, double gamma, double *bias_out);
int sfw_grid_blend_control(sfw_handle h, const double *lambda, int32_t L, double gamma, const double *bias,
                           sfw_blend_stat *stat_out, double *u_out, double *weights_out);

/* sfw_mppi_run: I = m->iterations iterations of perturb -> score -> control cost -> blend -> new nominal plan, enqueued
 * back to back behind ONE wait.  It is defined as this loop of the calls above and equals it BIT FOR BIT in every output:
 *   nom_0 = p->nominal
 *   for i = 0 .. I-1:
 *       pt = *p;  pt.seed = p->seed + i (mod 2^64);  pt.nominal = nom_i
 *       sfw_sequences_perturb_stage(h, rs, &pt, n, K, knot_step, args, 0);  sfw_grid_launch(h);
 *       sfw_grid_fetch(h, NULL, &best_i, NULL)
 *       sfw_grid_blend_control(h, &m->lambda, 1, m->gamma, NULL, &stat_out[i], u_i, NULL)
 *       nom_(i+1) = stat_out[i].n_valid > 0 ? u_i : nom_i
 *       plans_out[i] = nom_(i+1)                                      (K x 3 doubles: [k][vx, vy, vtheta])
 *   *best_out = best_(I-1)                                             (nullable)
 * Between iterations nothing goes through the host: a perturb kernel reads the plan from device memory, where the blend's
 * last kernel leaves the next one.  Afterwards the handle is exactly as after iteration I-1 of that loop — it holds a
 * perturbed stage drawn around nom_(I-1) with seed p->seed + I - 1, launched and fetched — and sfw_grid_costs_view,
 * sfw_grid_fetch, sfw_sequences_knots / _normals, sfw_grid_crowd, the terms and points capture, sfw_grid_rescore,
 * sfw_grid_blend(_control), sfw_sequences_control_cost, sfw_grid_plan_info and a re-launch act on that iteration.  Under
 * SFW_PERTURB_KEEP_NOMINAL sample 0 of iteration i is nom_i itself, so its cost is in the cost vector.  The plan is always
 * finite: a weighted mean of clamped knots, or the caller's checked nominal.
 * SFW_ERR_INVALID_ARG (before any device call; a refused call changes nothing): a NULL h, m, stat_out or plans_out;
 * iterations outside [1, SFW_MPPI_MAX_ITER]; reserved != 0; a lambda that is not finite or not > 0; a gamma that is not
 * finite; everything sfw_sequences_perturb_stage refuses at index_base 0.  SFW_ERR_STATE: no costmap.  Any later failure
 * leaves nothing staged or launched, as for every stage. */
#define SFW_MPPI_MAX_ITER 32
typedef struct sfw_mppi {
  int32_t iterations, reserved; /* 1 .. SFW_MPPI_MAX_ITER; 0 */
  double lambda;                /* the blend's temperature, finite, > 0 */
  double gamma;                 /* the control cost's factor, finite; 0: no control cost */
} sfw_mppi;
int sfw_mppi_run(sfw_handle h, const sfw_robot_state *rs, const sfw_perturb *p, int32_t n, int32_t K,
                 const int32_t *knot_step, const sfw_goal_args *args, const sfw_mppi *m,
                 sfw_blend_stat *stat_out /* I */, double *plans_out /* I x K x 3 */, sfw_best *best_out /* nullable */);

/* ---- the predicted crowd behind a score ------------------------------------
 * For every sample the scorer integrates the whole crowd forward under the social-force model; these two calls hand that
 * prediction out for ONE sample: where every person is after every step, who does the social work, whose goal has popped.
 * One wave integrates the sample once more (K1 + a capturing form of the flat K2 + one device-to-host copy of
 * 16 + 44 * steps * agents bytes); the values are the scoring kernels' own, in all three precision modes.
 *
 * The pedestrian prediction behind ONE scoreTrajectory call.  Row i (0 <= i < *n_steps) is the world AFTER Euler step i:
 *   state[(i*A + a)*4 + 0..3] = x, y, vx, vy of agent a.  a = 0 is the robot as the reference overwrites it after the step
 *       (ref :600-604): position = Trajectory pose i+1, velocity = the robot-local twist (vx_i, vy_i);
 *   work[i*A + a]     a = 0: Wr of step i = |social force| + |obstacle force| on the robot at the PRE-step state (ref :681-682);
 *                     a >= 1: |force the post-step robot alone exerts on person a| (ref :692-699), 0.0 for a person whose id
 *                     is the robot's.  Summed over a and i these ARE the sample's social-work term (SFW_TERM_SOCIAL); only a
 *                     person's entry below 1e-140 (SFW_PRECISION_F32: 1e-12), which that sum's norm cannot resolve, is
 *                     evaluated apart from it, in double;
 *   has_goal[i*A + a] 1 while person a's goal has not been popped after step i (a = 0: 0).
 * *n_steps = steps the reference integrates before it returns = the Trajectory point count sfw_score_one reports for the same
 * call: S for a valid sample, c + 1 for a pedestrian contact at step c (row c is the contact state), j for a footprint that
 * turns illegal at pose j (fewer if a contact comes first), 0 without agents.  At most steps_cap rows are written;
 * *n_steps is the full count.  work / has_goal are nullable.  agents must equal the agent count of the world the call
 * scores (SFW_ERR_INVALID_ARG otherwise, nothing written).  cost_out is bit for bit sfw_score_one's.
 * SFW_ERR_INVALID_ARG (before any device call): a NULL handle, cost_out, state_xyvv or n_steps, steps_cap < 1, a wrong
 * `agents`, and whatever sfw_score_one refuses; SFW_ERR_UNSUPPORTED: an agent set that does not fit one wave's LDS.  The
 * call consumes the staged grid exactly as sfw_score_one does. */
int sfw_score_one_crowd(sfw_handle h, const sfw_robot_state *rs, double vx_samp, double vy_samp, double vtheta_samp,
                        const sfw_goal_args *args, double *cost_out, double *state_xyvv, double *work, int32_t *has_goal,
                        int32_t agents, int32_t steps_cap, int32_t *n_steps);
/* The same for sample `index` of the staged grid or list (the winner: sfw_best.index), under the state rules of
 * sfw_grid_points: needs a stage (SFW_ERR_STATE otherwise), works before or after the launch and on batch / ensemble
 * members after their fetch, read-only for the launch (cost vector, selection, captured points and terms,
 * sfw_grid_rescore stay valid).  cost_out is nullable here.
 * The grid loop's skipped (0,0) sample: *n_steps = 0, *cost_out = SFW_COST_SKIPPED. */
int sfw_grid_crowd(sfw_handle h, int64_t index, double *cost_out, double *state_xyvv, double *work, int32_t *has_goal,
                   int32_t agents, int32_t steps_cap, int32_t *n_steps);

/* ---- one process, several devices ---------------------------------------
 * The reference plugin is ONE process (sfw_plugin.xml:1-9; computeVelocityCommands,
 * src/sfw_planner_node.cpp:220-331), so a host that wants the (v,w) grid on several
 * MI355X drives them from there: one sfw_handle per listed device, the linvel rows
 * (the OUTER loop of src/sfw_planner.cpp:345) split into R contiguous blocks of equal
 * planned work (sfw_plan_row_blocks; [r*nv/R, (r+1)*nv/R) when the shared-prefix rollout
 * has nothing to share), world state replicated by each handle's own upload, and the
 * winner picked by ONE ncclAllReduce(min) over xGMI of an [R,5] double table in which
 * rank r fills its own row (sfw_best_key + n_valid) and +inf elsewhere — the
 * lexicographic row minimum is the reference's selection order (:394-414).  RCCL is
 * loaded on first use (dlopen librccl.so): single-device callers never touch it. */
typedef struct sfw_multi_s *sfw_multi_handle;
#define SFW_MULTI_RCCL 0        /* devices must be distinct; exchange = ncclAllReduce(min)            */
#define SFW_MULTI_HOST_REDUCE 1 /* exchange on the host from each rank's 40-byte row: no RCCL needed, a
                                   device may be listed more than once (tests on a one-GPU box)       */
int sfw_multi_create(const sfw_params *params, const int *devices, int32_t R, int32_t exchange,
                     sfw_multi_handle *out);
int sfw_multi_destroy(sfw_multi_handle m);
const char *sfw_multi_last_error(sfw_multi_handle m);
int32_t sfw_multi_ranks(sfw_multi_handle m);
/* What the handle really runs on (diagnostics; a scaling record must say what it measured): the devices as listed, the
 * exchange, and — SFW_MULTI_RCCL — how many communicators ncclCommInitAll returned, the size communicator 0 reports
 * (ncclCommCount), the device every communicator reports (ncclCommCuDevice) and RCCL's version code (ncclGetVersion);
 * -1 / 0 where the library does not export the query.  At most the first 64 ranks are listed. */
typedef struct sfw_multi_desc {
  int32_t ranks, exchange, communicators, comm_size, rccl_version;
  int32_t devices[64], comm_devices[64];
  /* SFW_MULTI_RCCL: the file ncclAllReduce was resolved from (dladdr) and how it was found — "SFW_RCCL_LIB" (that path in
   * the environment, honoured first), "already mapped" (an RCCL this process had loaded — e.g. the copy torch bundles — is
   * reused rather than a second one opened beside it) or the name the loader was given (librccl.so, librccl.so.1,
   * /opt/rocm/lib/librccl.so).  Empty strings for SFW_MULTI_HOST_REDUCE. */
  char rccl_path[512], rccl_found[64];
} sfw_multi_desc;
int sfw_multi_describe(sfw_multi_handle m, sfw_multi_desc *out);
/* Rank r's handle (owned by m): for the single-sample calls (sfw_score_one on rank 0) and diagnostics. */
sfw_handle sfw_multi_rank_handle(sfw_multi_handle m, int32_t r);
/* World state and parameters, replicated to every rank. */
int sfw_multi_set_params(sfw_multi_handle m, const sfw_params *params);
int sfw_multi_set_costmap(sfw_multi_handle m, const uint8_t *cells, uint32_t size_x, uint32_t size_y,
                          double origin_x, double origin_y, double resolution);
int sfw_multi_set_footprint(sfw_multi_handle m, const double *xy, int32_t K);
int sfw_multi_set_agents(sfw_multi_handle m, const sfw_agent *agents, int32_t A, const double *obstacles_xy,
                         int32_t O);
/* sfw_score_grid over all ranks: same arguments, same results (costs bit-identical: a sample's cost does
 * not depend on how the grid is cut).  costs_out / best_out may be NULL. */
int sfw_multi_score_grid(sfw_multi_handle m, const sfw_robot_state *rs, const double *linvels, int32_t nv,
                         const double *angvels, int32_t nw, const sfw_goal_args *args, double *costs_out,
                         sfw_best *best_out);
/* The block of rows rank r scored in the last sfw_multi_score_grid. */
int sfw_multi_rank_rows(sfw_multi_handle m, int32_t r, int32_t *first_row, int32_t *n_rows);
/* Host wall-clock of the last call's phases, microseconds: which = 0 stage+launch of all ranks (enqueue),
 * 1 exchange (enqueue of the all-reduce + fetch of the table, i.e. until every rank's kernels are done),
 * 2 cost-vector fetches. */
int sfw_multi_last_us(sfw_multi_handle m, int32_t which, double *us_out);
/* Trajectory points of sample `index` of the last sfw_multi_score_grid (as sfw_grid_points). */
int sfw_multi_grid_points(sfw_multi_handle m, int64_t index, double *points_xyth, int32_t points_cap,
                          int32_t *n_points);

/* ---- many planners in one launch ------------------------------------------
 * A fleet server scoring the local planners of many robots, or a harness stepping many scenes: B ordinary handles on one
 * device that share ONE stream (the batch's), scored together.  Every member is a full sfw_handle: set its parameters,
 * costmap, footprint and agents, stage its own grid (grids, step counts and precisions may differ), turn on points capture,
 * or score it alone, as for any handle; only destroying it is refused (SFW_ERR_STATE: the batch owns it).
 * sfw_batch_launch enqueues every member's staged grid: the members whose launch would be the one-kernel control cycle
 * (sfw_plan_info.one_launch) go through ONE launch of a batched cycle kernel per kernel variant (precision x groups x
 * laser points: a homogeneous fleet is one launch), the others through their usual kernels behind it on the same stream.
 * Every member's results (costs, sentinels, selection, captured Trajectory points, contact steps) are bit-identical to
 * its own launch, and after sfw_batch_fetch sfw_grid_costs_view / sfw_grid_fetch / sfw_grid_points(_batch) of a member
 * behave as after that member's own launch.  Member timing (sfw_set_timing) is not recorded in a batch launch.
 * A member staged with a sample list, sequences or perturbed rollouts takes its own path by default.  Under the sticky switch
 * sfw_batch_set_list_fusion (off when the batch is created) such a member joins the batched launch too, when its own launch
 * would be the one-kernel cycle: the kernel variant is then stage kind (grid / list / sequences of more than one knot) x
 * precision x groups x laser points — a fleet of MPPI controllers with n <= 1024 rollouts each is ONE launch — and the member
 * counts under one_launch_members.  A member that does not qualify (more than 1024 samples, more steps than the small-rollout
 * limit, a crowd beyond the 64-double planes, SFW_CYCLE_FUSED=0, a chunked stage) keeps its own path.  A perturbed member's
 * draw is enqueued by its stage on the batch's stream, ahead of the launch.  Results are bit-identical either way. */
#define SFW_BATCH_MAX 256
typedef struct sfw_batch_s *sfw_batch;
/* 1 <= B <= SFW_BATCH_MAX; SFW_ERR_NO_DEVICE without a GPU, as sfw_create. */
int sfw_batch_create(const sfw_params *params, int device, int32_t B, sfw_batch *out);
int sfw_batch_destroy(sfw_batch b);
const char *sfw_batch_last_error(sfw_batch b);
int32_t sfw_batch_size(sfw_batch b);
/* Member i (owned by b; NULL when out of range). */
sfw_handle sfw_batch_member(sfw_batch b, int32_t i);
/* Every member must have a staged grid (a grid staged and consumed by a single-sample score counts as none): otherwise
 * SFW_ERR_STATE, nothing is enqueued, and the last error names the member.  No host sync. */
int sfw_batch_launch(sfw_batch b);
/* One wait for the whole batch; best_out (nullable) receives B selections in member order. */
int sfw_batch_fetch(sfw_batch b, sfw_best *best_out);
/* Stage member i with rs[i] and args[i] on the common grid (linvels x angvels), launch, fetch.  A failing stage launches
 * nothing. */
int sfw_batch_score_grid(sfw_batch b, const sfw_robot_state *rs, const double *linvels, int32_t nv,
                         const double *angvels, int32_t nw, const sfw_goal_args *args, sfw_best *best_out);
/* The sticky switch described above.  enabled != 0: on.  SFW_ERR_INVALID_ARG: b (or enabled_out) NULL. */
int sfw_batch_set_list_fusion(sfw_batch b, int32_t enabled);
int sfw_batch_get_list_fusion(sfw_batch b, int32_t *enabled_out);
/* The list forms of sfw_batch_score_grid: member i is staged with rs[i], args[i] and its OWN samples by the single stage's
 * function (sfw_samples_stage, sfw_sequences_stage, sfw_sequences_perturb_stage; index_base 0), then launch and fetch.  The
 * arrays are member-major: member i's knot k of sample t lies at [(i * K + k) * n + t] (K == 1 for samples); vy is nullable;
 * knot_step[K] is common; p holds B perturbations.  The argument rules are the single stage's, read for ALL members before any
 * member is staged: a call refused for its arguments (SFW_ERR_INVALID_ARG) changes nothing — the previous launch is still
 * fetchable —, and a failing stage launches nothing.  They honour sfw_batch_set_list_fusion; they do not turn it on. */
int sfw_batch_score_samples(sfw_batch b, const sfw_robot_state *rs, const double *vx, const double *vy, const double *vtheta,
                            int32_t n, const sfw_goal_args *args, sfw_best *best_out);
int sfw_batch_score_sequences(sfw_batch b, const sfw_robot_state *rs, const double *vx, const double *vy,
                              const double *vtheta, int32_t n, int32_t K, const int32_t *knot_step,
                              const sfw_goal_args *args, sfw_best *best_out);
int sfw_batch_score_perturbed(sfw_batch b, const sfw_robot_state *rs, const sfw_perturb *p /* [B] */, int32_t n, int32_t K,
                              const int32_t *knot_step, const sfw_goal_args *args, sfw_best *best_out);
/* What the last launch did: members that went through a batched launch, members on their own path, batched launches,
 * blocks over all batched launches and the largest dynamic LDS of a block among them (bytes). */
typedef struct sfw_batch_desc {
  int32_t members, one_launch_members, own_path_members, batch_launches;
  int64_t batch_blocks;
  int32_t lds_bytes;
} sfw_batch_desc;
int sfw_batch_describe(sfw_batch b, sfw_batch_desc *out);
/* Host wall-clock of the last calls, microseconds: which = 0 staging of the last batch score (that call only), 1 the
 * enqueue of the last launch, 2 the wait and fetch of the last fetch. */
int sfw_batch_last_us(sfw_batch b, int32_t which, double *us_out);

/* ---- one grid under several crowd hypotheses ------------------------------
 * The reference gives every person the goal position + naive_goal_time * velocity (src/sensor_interface.cpp:491-502): one
 * guess of where the crowd is heading.  An ensemble scores one robot's grid under M hypotheses of the crowd and picks the
 * command that is best on average over them, or best in the worst of them.  All hypotheses share the parameters, costmap,
 * footprint, robot state, goal arguments and (v, w) grid; each has its own agents (agents[0] = the robot in every one; the
 * number of people may differ) and laser points.  Member m scores the grid exactly as a standalone handle would, with terms
 * captured (sfw_set_terms_capture); then, for sample t, with tau_m[k][t] member m's terms and w the ensemble's weights:
 *   - the (0,0) sample is SFW_COST_SKIPPED in every member: ensemble cost SFW_COST_SKIPPED, rejected[t] = 0;
 *   - rejected[t] = members whose cost is SFW_COST_INVALID; rejected[t] > 0: ensemble cost SFW_COST_INVALID (contact in any
 *     hypothesis rejects the command).  Costmap rejection does not depend on the agents: rejected[t] == M covers it, and
 *     0 < rejected[t] < M always means pedestrian contact in some crowds (a chance constraint is sfw_risk.contact_mass,
 *     "Risk" below);
 *   - otherwise the social work W_m is aggregated: SFW_ENSEMBLE_MEAN: acc = 0.0; acc = acc + p[m] * W_m for m = 0..M-1 in
 *     that order, each product and sum rounded on its own (p: caller-given, finite, >= 0, need not sum to 1; NULL: 1.0 / M
 *     each); SFW_ENSEMBLE_MAX: the largest W_m (worst case).  The cost is the scoring kernels' own combination of member 0's
 *     pedestrian-free terms (velocity, distance, angle, costmap: the same in every member that accepts the sample) and the
 *     aggregate, so M = 1 with p = {1} reproduces the member's cost bit for bit.
 * Selection is the reference's rule (the 10000.0 cap, the tie-breaks) over the ensemble cost vector, index_base 0; n_valid
 * counts ensemble-valid samples. */
#define SFW_ENSEMBLE_MAX_M 64
#define SFW_ENSEMBLE_MEAN 0
#define SFW_ENSEMBLE_MAX 1
typedef struct sfw_ensemble_s *sfw_ensemble;
/* 1 <= M <= SFW_ENSEMBLE_MAX_M (else SFW_ERR_INVALID_ARG, before any device call); SFW_ERR_NO_DEVICE without a GPU. */
int sfw_ensemble_create(const sfw_params *params, int device, int32_t M, sfw_ensemble *out);
int sfw_ensemble_destroy(sfw_ensemble e);
const char *sfw_ensemble_last_error(sfw_ensemble e);
int32_t sfw_ensemble_size(sfw_ensemble e);
/* Member m (owned by e; NULL when out of range): its costs (sfw_grid_costs_view), terms (sfw_grid_terms) and Trajectory
 * points after a score, as a batch member's.  sfw_destroy of it is refused (SFW_ERR_STATE). */
sfw_handle sfw_ensemble_member(sfw_ensemble e, int32_t m);
/* Replicated to every member.  Parameters changed through a member handle make the next score SFW_ERR_STATE (a memcmp). */
int sfw_ensemble_set_params(sfw_ensemble e, const sfw_params *params);
int sfw_ensemble_set_costmap(sfw_ensemble e, const uint8_t *cells, uint32_t size_x, uint32_t size_y,
                             double origin_x, double origin_y, double resolution);
int sfw_ensemble_set_footprint(sfw_ensemble e, const double *xy, int32_t K);
/* Hypothesis m: a full sfw_set_agents input. */
int sfw_ensemble_set_hypothesis(sfw_ensemble e, int32_t m, const sfw_agent *agents, int32_t A,
                                const double *obstacles_xy, int32_t O);
/* Stage every member on the grid, ONE batch launch (sfw_batch_*: members that qualify for the one-launch cycle share a
 * batched cycle kernel, the others take their usual kernels on the same stream), the aggregation kernel behind it, one wait.
 * costs_out (nv * nw doubles), rejected_out (nv * nw int32) and best_out are nullable.  SFW_ERR_INVALID_ARG for an unknown
 * mode or a non-finite or negative probability (checked before any device call); SFW_ERR_STATE when a hypothesis was never
 * set or a member's sfw_params differ from the ensemble's. */
int sfw_ensemble_score_grid(sfw_ensemble e, const sfw_robot_state *rs, const double *linvels, int32_t nv,
                            const double *angvels, int32_t nw, const sfw_goal_args *args, int32_t mode,
                            const double *probs, double *costs_out, int32_t *rejected_out, sfw_best *best_out);
/* Re-aggregate the last score under another mode / probabilities, no rollout: one kernel over the members' captured terms.
 * Same argument checks; SFW_ERR_STATE when nothing was scored, or when a member was staged, launched or used for
 * sfw_score_one since (the rule of sfw_grid_rescore). */
int sfw_ensemble_aggregate(sfw_ensemble e, int32_t mode, const double *probs, double *costs_out,
                           int32_t *rejected_out, sfw_best *best_out);
/* The same over n command SEQUENCES of K knots instead of a grid (MPPI rollouts under crowd uncertainty).  Every member
 * stages the same sequences as sfw_sequences_stage would (vx / vy (nullable) / vtheta: K rows of n values, knot-major;
 * index_base 0), one batch launch, the aggregation behind it, one wait: the shape of sfw_ensemble_score_grid.  K == 1 is a
 * sample list (sfw_samples_stage).  Afterwards member m is as after its own sfw_score_sequences: costs view, terms, points,
 * sfw_grid_crowd, sfw_sequences_knots.  The aggregation is the definition above, unchanged; a list has no skipped sample, so
 * SFW_COST_SKIPPED never appears.  Selection is the LIST's rule over the ensemble cost vector: the first knot's vx and
 * vtheta are the key's velocities (vy takes no part), the larger index wins among equals; best_out carries the winner's
 * first knot.  costs_out (n doubles), rejected_out (n int32) and best_out are nullable.
 * Refusals, in this order: mode and probabilities as sfw_ensemble_score_grid; then every argument rule of
 * sfw_sequences_stage (SFW_ERR_INVALID_ARG) — before any member is staged, so the previous score stays usable by
 * sfw_ensemble_aggregate and sfw_ensemble_blend; then SFW_ERR_STATE when a hypothesis was never set, a member's sfw_params
 * differ, its terms capture was turned off or no costmap was set.  A failure from there on leaves nothing scored.
 * sfw_ensemble_aggregate after this call re-aggregates with the list's selection. */
int sfw_ensemble_score_sequences(sfw_ensemble e, const sfw_robot_state *rs, const double *vx, const double *vy,
                                 const double *vtheta, int32_t n, int32_t K, const int32_t *knot_step,
                                 const sfw_goal_args *args, int32_t mode, const double *probs, double *costs_out,
                                 int32_t *rejected_out, sfw_best *best_out);
/* ... with the knots drawn on the device: every member stages as sfw_sequences_perturb_stage would with the same *p and
 * index_base 0, so all members hold bitwise the same knots (sfw_sequences_knots on any member) and the results are those of
 * sfw_ensemble_score_sequences fed these knots.  best_out's command is read from the device.  The argument rules are those
 * of sfw_sequences_perturb_stage, in the same place. */
int sfw_ensemble_score_perturbed(sfw_ensemble e, const sfw_robot_state *rs, const sfw_perturb *p, int32_t n, int32_t K,
                                 const int32_t *knot_step, const sfw_goal_args *args, int32_t mode, const double *probs,
                                 double *costs_out, int32_t *rejected_out, sfw_best *best_out);
/* sfw_grid_blend over the ENSEMBLE cost vector: its definition, its outputs and its summation tree ("Determinism" above),
 * with J_t the cost vector of the last aggregation (a score call or sfw_ensemble_aggregate) and the knots of member 0 — after
 * sfw_ensemble_score_grid K = 1 and sample t = iv * nw + iw, as the handle's blend over a grid.  Read-only for the score: it
 * may be repeated and alternate with sfw_ensemble_aggregate.  stat.n_valid is best.n_valid of that aggregation; with no valid
 * sample the all-zero record of sfw_grid_blend comes back with SFW_OK.  The cost vector is read on the device wherever the
 * aggregation left it for the host.  Argument refusals are sfw_grid_blend's (before any device call); SFW_ERR_STATE by the
 * rule of sfw_ensemble_aggregate.  Member 0's own sfw_grid_blend is not disturbed: the ensemble has buffers of its own. */
int sfw_ensemble_blend(sfw_ensemble e, const double *lambda, int32_t L, const double *bias, sfw_blend_stat *stat_out,
                       double *u_out, double *weights_out);
/* sfw_ensemble_blend with the control cost: J_t = cost_t + b_t, where b_t = gamma * c_t (bias == NULL) or (gamma * c_t) +
 * bias_t, and c_t is the "Control cost" of member 0's perturbed stage (every member staged the same sfw_perturb).  Nothing
 * else differs — the definition, the outputs, the summation tree and the state rule are sfw_ensemble_blend's: what
 * sfw_grid_blend_control is to sfw_grid_blend.  The bias vector never leaves the device, and lives in a buffer of the
 * ensemble's: member 0's own sfw_grid_blend_control is not disturbed, nor the other way round.  gamma == 0 is bit for bit
 * sfw_ensemble_blend with the same `bias`.  SFW_ERR_STATE: sfw_ensemble_blend's rule, and when the last score was not a
 * perturbed one (sfw_ensemble_score_perturbed, sfw_ensemble_mppi_run).  SFW_ERR_INVALID_ARG (before any device call; a
 * refused call changes nothing): what sfw_ensemble_blend refuses, and a gamma that is not finite. */
int sfw_ensemble_blend_control(sfw_ensemble e, const double *lambda, int32_t L, double gamma, const double *bias,
                               sfw_blend_stat *stat_out, double *u_out, double *weights_out);
/* sfw_mppi_run under M crowd hypotheses: I = m->iterations iterations of perturb -> score all members -> aggregate -> control
 * cost -> blend -> new nominal plan, enqueued back to back on the ensemble's stream behind ONE wait.  It is defined as this
 * loop of the calls above and equals it BIT FOR BIT in every output:
 *   nom_0 = p->nominal
 *   for i = 0 .. I-1:
 *       pt = *p;  pt.seed = p->seed + i (mod 2^64);  pt.nominal = nom_i
 *       sfw_ensemble_score_perturbed(e, rs, &pt, n, K, knot_step, args, mode, probs, costs_i, rejected_i, &best_i)
 *       sfw_ensemble_blend_control(e, &m->lambda, 1, m->gamma, NULL, &stat_out[i], u_i, NULL)
 *       nom_(i+1) = stat_out[i].n_valid > 0 ? u_i : nom_i
 *       plans_out[i] = nom_(i+1)                                      (K x 3 doubles: [k][vx, vy, vtheta])
 *   costs_out = costs_(I-1);  rejected_out = rejected_(I-1);  *best_out = best_(I-1)        (n, n, one: each nullable)
 * Iteration 0 stages the members as sfw_ensemble_score_perturbed does.  From there nothing goes through the host: ONE kernel
 * (sfw_perturb_members_kernel) draws each knot once around the plan in device memory and stores it into every member's rows,
 * the members' kernels and the aggregation follow, and the blend's last kernel leaves the next plan where the next draw
 * reads it.  Afterwards the ensemble and every member are exactly as after iteration I-1 of that loop: sfw_ensemble_aggregate,
 * sfw_ensemble_blend(_control), a member's costs view, terms, points, sfw_sequences_knots / _normals and sfw_grid_crowd act on
 * that iteration, and every member remembers nom_(I-1) and seed + I - 1 as what it was drawn from.
 * Refusals, in this order (all SFW_ERR_INVALID_ARG, before any member is staged, so the previous score stays usable): mode and
 * probabilities; m NULL, iterations outside [1, SFW_MPPI_MAX_ITER], reserved != 0, a lambda that is not finite or not > 0, a
 * gamma that is not finite; a NULL stat_out or plans_out; everything sfw_ensemble_score_perturbed refuses.  Then SFW_ERR_STATE
 * as for every ensemble score.  Any later failure leaves nothing scored, and every member with nothing staged or launched. */
int sfw_ensemble_mppi_run(sfw_ensemble e, const sfw_robot_state *rs, const sfw_perturb *p, int32_t n, int32_t K,
                          const int32_t *knot_step, const sfw_goal_args *args, int32_t mode, const double *probs,
                          const sfw_mppi *m, sfw_blend_stat *stat_out /* I */, double *plans_out /* I x K x 3 */,
                          double *costs_out /* n, nullable */, int32_t *rejected_out /* n, nullable */,
                          sfw_best *best_out /* nullable */);
/* ---- Risk: a tail expectation (CVaR) of the social work and a bound on the contact mass ----
 * Sticky state of the ensemble, off by default.  While it is off every call does exactly what is written above.  While it is
 * set, EVERY aggregation reads it — the three score calls, sfw_ensemble_aggregate and every iteration of
 * sfw_ensemble_mppi_run — and `mode` keeps its two values.  sfw_ensemble_set_risk makes no device call and does not
 * invalidate the last score: sfw_ensemble_aggregate after it re-aggregates under the new setting (a risk sweep over one scored
 * grid costs a launch and a wait per setting, no rollout).  r == NULL turns it off.  A refused call keeps the previous setting.
 *
 * Once per aggregation, on the host: p[m] the caller's probability, or 1.0 / M when probs is NULL;
 * P = ((0.0 + p[0]) + p[1]) + ... in member order; thr = contact_mass * P (one product).
 * Per sample t, with d_m member m's distance term and W_m its social work; all arithmetic in double, every product, sum and
 * quotient rounded on its own (no contraction), loops in member order unless stated:
 *   1. any member SFW_COST_SKIPPED: cost SFW_COST_SKIPPED, rejected[t] = 0 (grids only; unchanged);
 *   2. rejected[t] = members with d_m == SFW_COST_INVALID (unchanged);
 *   3. R = the sum of p[m] over the rejecting members, Pa = the sum over the accepting members, both from +0.0;
 *   4. the cost is SFW_COST_INVALID when rejected[t] == M; or contact_mass == 0 and rejected[t] > 0 (the rule above, bit for
 *      bit); or contact_mass > 0 and R > thr; or Pa == 0;
 *   5. otherwise the aggregate A is
 *        SFW_ENSEMBLE_MAX:  the largest W_m over the ACCEPTING members (tail_mass is not read);
 *        SFW_ENSEMBLE_MEAN: tau = tail_mass * Pa; rem = tau; acc = +0.0; the accepting members are visited by W_m descending,
 *          the lower member index first among equal W_m; for each: take = min(p[m], rem); acc = acc + take * W_m;
 *          rem = rem - take; finally A = acc / tau.  (Once rem == 0 every later member adds +0.0: stopping there changes no
 *          bit, and the kernel stops there.)
 *   6. the cost is the scoring kernels' own combination of the pedestrian-free terms of the LOWEST-INDEXED ACCEPTING member and
 *      A.
 * Selection, n_valid, the blend and the MPPI chain read this cost vector as they read the plain one.  Consequences:
 *   - M = 1, p = {1}, tail_mass = 1, contact_mass = 0 is the member's cost bit for bit;
 *   - tail_mass = 1 is the NORMALISED mean (divided by Pa): it equals the plain SFW_ENSEMBLE_MEAN only to rounding, and only
 *     when the probabilities sum to 1;
 *   - a tail_mass no larger than the worst member's share is SFW_ENSEMBLE_MAX to within two roundings ((tau * W) / tau);
 *   - under contact_mass > 0 a sample may be valid although member 0 rejects it: its cost then comes from another member's
 *     terms, and `rejected[t]` still counts the rejecting members.
 * SFW_ERR_INVALID_ARG: e NULL (setter and getter; the getter also for out NULL); a tail_mass that is not finite or outside
 * (0, 1]; a contact_mass that is not finite or outside [0, 1); reserved != 0.  While a risk is set every aggregating call
 * refuses P == 0 (all probabilities zero) with SFW_ERR_INVALID_ARG, where it checks the mode and the probabilities: before any
 * member is staged, so the previous score stays usable. */
typedef struct sfw_risk {
  double tail_mass;    /* finite, 0 < tail_mass <= 1: share of the (accepted) probability mass, worst social work first */
  double contact_mass; /* finite, 0 <= contact_mass < 1: share of the probability mass that may end in contact         */
  int64_t reserved;    /* 0 */
} sfw_risk;
int sfw_ensemble_set_risk(sfw_ensemble e, const sfw_risk *r); /* NULL: off (the default) */
/* *out: the setting (tail_mass 1, contact_mass 0 while off); *active_out (nullable): 1 while a risk is set, else 0. */
int sfw_ensemble_get_risk(sfw_ensemble e, sfw_risk *out, int32_t *active_out);
/* sfw_batch_set_list_fusion of the ensemble's private batch (off by default): with it on, sfw_ensemble_score_sequences,
 * _score_perturbed and every iteration of sfw_ensemble_mppi_run score the M members in one batched launch (per kernel variant)
 * instead of M launches; the chain uploads the member table in iteration 0 and launches again from the device copy while an
 * iteration's records are the bytes last uploaded.  Bit-identical results either way. */
int sfw_ensemble_set_list_fusion(sfw_ensemble e, int32_t enabled);
int sfw_ensemble_get_list_fusion(sfw_ensemble e, int32_t *enabled_out);
/* sfw_batch_describe of the private batch's last launch (SFW_ERR_STATE before any); *table_uploads_out (nullable): member-table
 * uploads of the last sfw_ensemble_mppi_run's launches (0 without list fusion). */
int sfw_ensemble_batch_desc(sfw_ensemble e, sfw_batch_desc *out, int64_t *table_uploads_out);
/* Host wall-clock of the last calls, microseconds: which = 0 staging of the members (the score calls only), 1 the enqueue of
 * the launch and the aggregation, 2 the wait and the copies out. */
int sfw_ensemble_last_us(sfw_ensemble e, int32_t which, double *us_out);

/* ---- the stop check: reject samples that cannot brake to a stop ---------------------------------------------------
 * The dynamic window's admissibility test (reference SFWPlanner::mayIStop, sfw_planner.hpp:348, src/sfw_planner.cpp
 * :717-765; its call at the end of scoreTrajectory, :636-640, is commented out there).  Off by default: with it off no
 * kernel is added to a launch and every output is bit-identical to a build without it.
 *
 * With a check set, a sample whose rollout poses were all legal (VALID behind the costmap scan) is braked from the state
 * the rollout left — (x_S, y_S, th_S) and the velocities of step S - 1 — with the rollout's own dt:
 *     j = 0
 *     while (vx != 0 || vy != 0):
 *         if j == max_steps: hit = SFW_STOP_UNFINISHED; reject
 *         vx  = new_velocity(0, vx,  dec_x, dt);  vy = new_velocity(0, vy, dec_y, dt);  vth = new_velocity(0, vth, dec_theta, dt)
 *         x  += (vx cos(th) + vy cos(pi/2 + th)) dt;  y += (vx sin(th) + vy sin(pi/2 + th)) dt    (OLD heading, the rollout's
 *         th += vth dt                                                        expressions; the lateral term only when vy != 0)
 *         code = footprint cost of (x, y, th)                     (the post-step pose at its NEW heading; off the map: -3)
 *         if code < 0 || code >= 254: hit = min(hit, j)
 *         j++
 *     steps = j
 * steps is the length of the whole tail, hit the first illegal tail pose or SFW_STOP_NONE.  A sample with a hit (or
 * UNFINISHED) is rejected exactly like a costmap rejection behind S legal poses: cost SFW_COST_INVALID, captured terms
 * -1, not counted in n_valid, never selected, not integrated with the pedestrians (except for the point dumps, as
 * before); its Trajectory keeps its S points.  Pedestrians play no part in the tail, as in the reference.  No
 * contraction in this arithmetic, as in the rest of the robot's rollout: the result does not depend on which kernels ran.
 *
 * Where this departs from the reference's (dead) code, on purpose:
 *   1. the reference hands `av`, the angular velocity, to computeNewXPosition / computeNewYPosition in the heading's place
 *      (:734-735); here it is the heading, the evident intent;
 *   2. the reference loops while the velocities are `> 0.0` and so never checks a reversing robot; here the condition is != 0;
 *   3. the reference loops for ever at a zero limit; here max_steps ends the loop and the sample is rejected.
 * A limit of exactly 0 is accepted: that axis never brakes, and a sample still moving on it ends UNFINISHED.
 *
 * The setting is sticky and per handle, and is read by the next stage; a launch of a grid staged earlier keeps what it was
 * staged with (as with sfw_set_costmap).  It reaches sfw_score_one, the sample lists, sequences, perturbed rollouts,
 * sfw_mppi_run and sfw_grid_rescore through the stage.  A stage with the check on never runs as the one-launch control
 * cycle (sfw_plan_info.one_launch = 0; a batch member with the check on takes its own path): the tail is not part of that
 * kernel yet.
 * Refused with SFW_ERR_INVALID_ARG, the handle keeping what it had: a NULL handle; a limit that is not finite or below 0;
 * max_steps outside 1 .. SFW_STOP_MAX_STEPS; reserved != 0. */
#define SFW_STOP_MAX_STEPS 4096
#define SFW_STOP_NONE (-1)       /* every tail pose legal */
#define SFW_STOP_UNFINISHED (-2) /* still moving after max_steps tail steps: rejected */
#define SFW_STOP_NOT_RUN (-3)    /* skipped, or rejected before the tail (costmap) */
typedef struct sfw_stop_check {
  double dec_x, dec_y, dec_theta; /* braking limits; the reference passes max_trans_acc_, max_trans_acc_, max_rot_acc_ */
  int32_t max_steps;              /* 1 .. SFW_STOP_MAX_STEPS */
  int32_t reserved;               /* 0 */
} sfw_stop_check;
typedef struct sfw_stop_rec {
  int32_t steps; /* length of the tail (0 when it did not run) */
  int32_t hit;   /* first illegal tail pose, or SFW_STOP_NONE / _UNFINISHED / _NOT_RUN */
} sfw_stop_rec;
int sfw_set_stop_check(sfw_handle h, const sfw_stop_check *c); /* NULL: off (the default) */
/* *out: the setting (all zero while off); *active_out (nullable): 1 while a check is set, else 0. */
int sfw_get_stop_check(sfw_handle h, sfw_stop_check *out, int32_t *active_out);
/* The records of samples [first, first + count) of the last launch (blocking).  SFW_ERR_STATE before a stage, before its
 * launch, and when the stage had the check off. */
int sfw_grid_stop_info(sfw_handle h, int64_t first, int64_t count, sfw_stop_rec *out);
/* The tail poses (x, y, theta) of samples [first, first + count) of the staged grid in check order — pose j is the one
 * hit == j refers to — by a re-run into scratch outputs that leaves the launch's results intact (RViz markers of the
 * braking path; blocking).  points_xyth: [count][steps_cap][3]; n_steps[i] is the full tail length even when it exceeds
 * steps_cap (0 for a sample whose tail did not run).  SFW_ERR_STATE before a stage and when the stage had the check off. */
int sfw_grid_stop_points(sfw_handle h, int64_t first, int64_t count, int32_t steps_cap, double *points_xyth, int32_t *n_steps);
/* The check of every member, like sfw_ensemble_set_footprint. */
int sfw_ensemble_set_stop_check(sfw_ensemble e, const sfw_stop_check *c);

/* ---- the path term: how far a rollout strays from the global plan --------------------------------------------------
 * A sixth cost term next to the reference's five: the mean squared distance of a sample's Trajectory points to the global
 * plan (the `path_distance_bias_ * path_cost` of the classic DWA sum, which the reference leaves in a comment at
 * src/sfw_planner.cpp:660-662 after reducing the plan to one way-point; DWB PathDist, the nav2 MPPI PathFollow critic).
 * Off by default: with no path set no kernel is added to a launch and every output is bit-identical to a build without it.
 *
 * A path is a polyline of n_points world points (1 .. SFW_PATH_MAX_POINTS) with n_points - 1 segments; a one-point path is
 * one zero-length segment.  Repeated points are legal (a zero-length segment).  The host turns each segment a -> b into a
 * record {ax, ay, ex, ey, inv} in double, without contraction:
 *     ex = bx - ax;  ey = by - ay;  len2 = ex*ex + ey*ey;  inv = len2 > 0 ? 1.0/len2 : 0.0
 * For a pose (px, py) and one segment, every operation rounded once, no FMA (the rule of the robot's rollout):
 *     rx = px - ax;  ry = py - ay
 *     u  = (rx*ex + ry*ey) * inv
 *     t  = u < 0 ? 0 : (u > 1 ? 1 : u)
 *     qx = rx - t*ex;  qy = ry - t*ey
 *     d  = qx*qx + qy*qy
 * D(pose) = min over segments of d, the running minimum `d < m ? d : m` from m = +inf: a minimum of doubles, exact in any
 * order.  The path term of a sample is the mean over the S points of its Trajectory — poses 0 .. S-1, the very doubles
 * sfw_grid_points returns —, summed in step order:
 *     p = (((D_0 + D_1) + D_2) + ... + D_{S-1}) / S
 * Pose 0 is the robot's own pose and adds the same constant to every sample; that is documented, not special-cased.
 * p is defined for every sample that is VALID behind the costmap scan (and behind the stop check when that is on); it does
 * not depend on the pedestrians: a sample rejected by contact keeps its p and has a sentinel cost.
 * The cost of a sample whose cost is not a sentinel becomes cost5 + path_weight * p — one multiply and one add, each rounded
 * once, behind the reference's five-term sum (a cost that equals SFW_COST_INVALID counts as that sentinel).  Sentinels stay;
 * n_valid, the cost == 10000.0 rule and the tie-breaks act on the new cost.  The captured terms stay the five (SFW_N_TERMS):
 * p lives in a buffer of its own, 8 B per sample, that exists only while a path is staged; the distance table adds 8 B per
 * step and sample to what SFW_TABLE_BUDGET_MB chunks.
 *
 * The setting is sticky and per handle and is read by the next stage (the points are copied); a launch of a grid staged
 * earlier keeps what it was staged with.  It reaches sfw_score_grid, sfw_score_one (the cost includes the term), sample
 * lists, sequences, perturbed rollouts, sfw_grid_blend* (they read the cost vector) and sfw_mppi_run through the stage.  A
 * stage with a path never runs as the one-launch control cycle (sfw_plan_info.one_launch = 0; a batch member with a path takes
 * its own path, sfw_batch_desc.own_path_members): the term is not part of that kernel.  sfw_multi_* has no wrapper: rank
 * handles take sfw_set_path one by one.
 * Refused with SFW_ERR_INVALID_ARG, the handle keeping what it had: a NULL handle or NULL xy; n_points outside
 * 1 .. SFW_PATH_MAX_POINTS; a coordinate that is not finite or exceeds SFW_PATH_MAX_COORD in magnitude (so that no product
 * overflows for an on-map pose); a weight that is not finite (a negative weight is accepted, as elsewhere); reserved != 0. */
#define SFW_PATH_MAX_POINTS 1024
#define SFW_PATH_MAX_COORD 1e7
typedef struct sfw_path {
  const double *xy; /* n_points x (x, y) */
  int32_t n_points; /* 1 .. SFW_PATH_MAX_POINTS */
  int32_t reserved; /* 0 */
  double weight;    /* path_weight */
} sfw_path;
int sfw_set_path(sfw_handle h, const sfw_path *p); /* NULL: off (the default) */
/* The setting in force for the next stage: up to cap points into xy_out (nullable when cap is 0), *n_points_out the number
 * the path has (0 while off), *weight_out, *active_out (each nullable). */
int sfw_get_path(sfw_handle h, double *xy_out, int32_t cap, int32_t *n_points_out, double *weight_out, int32_t *active_out);
/* The unweighted p of samples [first, first + count) of the last launch (blocking).  A sample rejected before or at the path
 * pass: SFW_COST_INVALID; the grid's (0,0) sample: SFW_COST_SKIPPED.  SFW_ERR_STATE before a stage, before its launch, and
 * when the stage had no path. */
int sfw_grid_path_term(sfw_handle h, int64_t first, int64_t count, double *out);
/* sfw_grid_rescore keeps its contract — what sfw_score_grid would return with these weights —: with a path staged it adds the
 * staged path_weight * p, and costs_out is bit-identical to that call's cost vector.  sfw_grid_rescore_path sweeps the sixth
 * weight over one launch: K path weights (NULL: the staged weight, K times) under the one weight vector *w; best_out K
 * records, costs_out (nullable) K x samples doubles, weight-major.  The rules of sfw_grid_rescore (K in
 * 1 .. SFW_RESCORE_MAX_K, finite weights, a launch with terms captured), and SFW_ERR_STATE when the stage had no path. */
int sfw_grid_rescore_path(sfw_handle h, const sfw_weights *w, const double *path_weight, int32_t K, sfw_best *best_out,
                          double *costs_out);
/* The path of every member, like sfw_ensemble_set_stop_check.  All members share robot state, map and path, so p is
 * bit-identical across members; every aggregation (mean / worst / under a risk; grids and lists, hence
 * sfw_ensemble_score_sequences, _score_perturbed, _aggregate, _blend* and _mppi_run) adds path_weight * p[t], taken from
 * member 0, behind the aggregated five-term cost and in front of the selection — also for a sample that member 0 rejects by
 * contact and a risk with contact_mass > 0 accepts.  Members whose path settings differ (one set through
 * sfw_ensemble_member): the scoring call returns SFW_ERR_STATE. */
int sfw_ensemble_set_path(sfw_ensemble e, const sfw_path *p);

#ifdef __cplusplus
}
#endif
#endif /* SFW_HIP_H_ */
