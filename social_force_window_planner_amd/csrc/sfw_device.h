// sfw_device.h — internal contract between the C-ABI host code (sfw_capi.hip)
// and the gfx950 kernels (sfw_kernels.hip).  Not part of the public ABI.
#ifndef SFW_DEVICE_H_
#define SFW_DEVICE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sfw_hip.h"

// The pair term's angular part is exactly 0 for a pair whose w x diff is exactly 0 — sign(theta) = 0, as in lightsfm for
// theta == 0 — at every step (a compare and one integer select per pair evaluation, exp2_fast2_gated); the host evaluates the
// reference's rounding-noise term for such pairs of the handed-over state (sfw_capi.hip rest_forces).

// Device shape the launch heuristics default to (a whole MI355X: 256 compute units in 8 XCDs of 32); a handle reads its
// device's own (hipDeviceProp_t.multiProcessorCount) and carries it into every launch (sfw_launch.n_cu / n_xcd).
#define SFW_DEFAULT_CUS 256
#define SFW_CUS_PER_XCD 32

// Per-sample status written by the rollout kernel.
enum : int32_t { SFW_ST_VALID = 0, SFW_ST_INVALID = 1, SFW_ST_SKIPPED = 2 };

// Post-step robot agent state for one (step, sample): what the reference
// writes into myagents[0] at src/sfw_planner.cpp:600-604 (position and the
// robot-LOCAL velocity).  32 bytes: the form a K2 wave holds it in (LDS).
struct __attribute__((aligned(32))) sfw_robot_step {
  double x, y, vx, vy;
};

// Pre-step footprint frame of one (step, sample): position and cos/sin(theta).
struct __attribute__((aligned(32))) sfw_pose_frame {
  double x, y, c, s;
};

// The K1 -> K2 / K1b tables in memory (round 6; rounds 1-5 stored the two 32-byte records above per (step, sample): 64 B).
// Of a robot step only the POSITION depends on both sample axes: the velocity sequence is the linear sample's alone
// (computeNewVelocity, ref :581-583), the heading — hence cos / sin — the angular sample's (ref :588), and the pose BEFORE
// step i is the position AFTER step i - 1.  So per step one row of 16-byte units
//     [ position after the step, one unit (x, y) per sample of the chunk | velocity (vx, vy) of the step, one unit per grid row ]
// (sfw_launch.ptab, row_units units per step) and one row (cos, sin) per grid column (sfw_launch.cs_tab): 16 B per (step,
// sample) written by the pose rollout and read back by K1b and K2 — a quarter of the traffic that bounded the rollout
// (cfg2: 42 MB in 16 us) — and a K2 lane still fetches its half of a record by ONE 16-byte load from a row base plus an
// offset that is fixed for the rollout.
struct __attribute__((aligned(16))) sfw_unit {
  double a, b;
};

// Person constants shared by every sample (device copy, SoA-friendly AoS).
struct __attribute__((aligned(16))) sfw_agent_const {
  double goal_x, goal_y;
  double goal_radius, desired_velocity;
  double radius;
  int32_t id, has_goal;
};

// Social-force constants derived from sfw_params on the host (sfw_derive), in the type the
// forces are evaluated in.  They reach the kernels as kernel arguments, i.e. in SGPRs: a value
// derived on the device (a division, a product) is a VALU result and would sit in a VGPR pair
// of every lane for the whole rollout.
template <typename R> struct sfw_force_k {
  // Everything that ends up in an exponent is in LOG2 units (the device evaluates 2^x, sfw_math.h): -log2(e)/gamma,
  // log2(Fs), c_vel = -(n' gamma)^2 log2(e), c_ang = -(n gamma)^2 log2(e), log2(k_obstacle), log2(e)/sigma
  R lambda, neg_l2e_inv_gamma, l2_f_social, c_vel, c_ang, l2_f_obstacle, l2e_inv_sigma;
};
struct sfw_derived {
  sfw_force_k<double> d;
  sfw_force_k<float> f;
  double f_desired, inv_tau, rr, inv_O;
  int32_t obs_tasks;  // flat K2, laser-point pass: 1 = (agent, segment) tasks over all lanes, 0 = one lane per agent
  int32_t obs_lds;    // flat K2: 1 = every wave keeps a copy of the laser points in LDS (set per launch by sfw_launch_social:
                      // launches that leave the GPU under-filled)
};

// Shared-prefix rollout (K2).  Under the acceleration limits the robot's first P steps are
// bit-identical for every sample of a CLASS (same clipped linear-velocity sequence x same clipped
// angular-velocity sequence up to the step before: the angular velocity of a step turns the heading
// the NEXT step moves along), hence so is the whole pedestrian simulation of those steps.  Classes
// refine as P grows, so the shared steps form a tree: level l simulates steps [P(l-1), P(l)) once per
// class of level l, each class resuming from the record its parent class (level l-1) left and leaving
// its own 64-byte record per agent; the suffix phase resumes every sample from its class of the last
// level for steps [P(last), S).  Same arithmetic on the same values in the same order: costs are
// bit-identical to the unshared rollout.
struct sfw_cls_agent {
  double px, py, vx, vy;  // state after the level's last step
  double fx, fy;          // desired + obstacle (+ group) force at that state = the next step's starting force
  double sw;              // the agent slot's social-work sum over the steps so far
  int32_t hasgoal, pad;
};
enum { SFW_PHASE_WHOLE = 0, SFW_PHASE_PREFIX = 1, SFW_PHASE_SUFFIX = 2 };

// The cost's linear combination (ref :663-667), shared by every kernel that forms a cost and by the re-score kernel
// (sfw_grid_rescore), so that a re-scored cost is bit-identical to a scored one.  The rounding is pinned here rather than
// left to -ffp-contract: the rollout kernels form the base terms and add the costmap term without contraction (K1 is
// compiled under fp contract(off)), and the social term is added by ONE fused multiply-add, fma(w_s, social, base), as
// every K2 epilogue has been compiled since round 1.
__device__ __forceinline__ double sfw_cost_base(double w_vel, double vel, double w_dist, double d, double w_ang, double ang) {
#pragma clang fp contract(off)
  return w_vel * vel + w_dist * d + w_ang * ang;
}
__device__ __forceinline__ double sfw_cost_add_costmap(double base, double w_costmap, double cm) {
#pragma clang fp contract(off)
  return base + w_costmap * cm;
}
__device__ __forceinline__ double sfw_cost_add_social(double base, double w_social, double social) {
  return __builtin_fma(w_social, social, base);
}

// Selection record (see sfw_best / sfw_best_key in the public header).
struct sfw_sel {
  double cost;       // +inf when nothing selectable
  double neg_linvel;
  double abs_angvel;
  long long neg_index;  // -(global iteration index)
  long long n_valid;
};

// One segment a -> b of the path (sfw_hip.h "the path term"): e = b - a, inv = 1 / |e|^2 or 0 for a zero-length segment,
// formed on the host (sfw_capi.hip path_segments).
struct sfw_path_seg {
  double ax, ay, ex, ey, inv;
};

// Everything the kernels need that is uniform over a launch.
struct sfw_launch {
  // scoring parameters
  sfw_params p;
  sfw_derived k;    // filled by sfw_derive
  int32_t S;        // num_steps
  double dt;        // sim_time / S
  // robot + goal
  sfw_robot_state rs;
  sfw_goal_args ga;
  double vy_samp;   // 0.0 for the grid loop
  int32_t skip_zero_sample;  // 1 for the grid loop (:349-352), 0 for score_one
  // samples: sample t = chunk_begin + local index; iv = t / nw, iw = t % nw
  const double *linvels;
  const double *angvels;
  int32_t nv, nw;
  int64_t chunk_begin;  // first sample of this chunk
  int64_t chunk_count;  // samples in this chunk
  // costmap snapshot
  const uint8_t *cells;
  uint32_t size_x, size_y;
  double origin_x, origin_y, resolution;
  const double *footprint;  // K x (x,y)
  int32_t K;
  // agents (index 0 = robot) and shared obstacle points
  const double *agent_pos;         // A x (x,y)
  const double *agent_vel;         // A x (vx,vy)
  const sfw_agent_const *agent_c;  // A
  const double *agent_rest;        // A x (fx, fy) or null: angular terms of the pairs at exact relative rest in the
                                   // handed-over state, evaluated on the host (sfw_capi.hip rest_forces)
  const double *pin_rest;          // 4 + A doubles or null: a person that can never move next to a robot that stands still for
                                   // the whole rollout is at exact relative rest at EVERY step; {robot x, y, lateral force on
                                   // the robot (x, y), Wp correction per person — 0 when the person is not pinned —} evaluated
                                   // on the host (sfw_capi.hip pinned_rest_table) for the steps whose robot record is (x, y)
                                   // at velocity 0; the kernels add entry 4 + i to person i's social work unconditionally
  int32_t A;
  const double *obstacles;         // O x (x,y)
  int32_t O;
  // groups of >= 1 agents with group_id >= 0 (dense index q, CSR member lists)
  const int32_t *agent_grp;        // A : dense group index or -1
  const int32_t *grp_off;          // NG + 1
  const int32_t *grp_mem;          // grp_off[NG] member agent indices, ascending per group
  int32_t NG;
  int32_t n_grp_mem;
  // shared-prefix rollout (see sfw_cls_agent); chunks are whole grid rows when phase != WHOLE.
  // Items of a PREFIX launch are the classes of one level (row class x column class; for a level ending at step p the row
  // classes of the first p linear velocities and the column classes of the first p - 1 angular ones — a robot record holds
  // the position, which takes the heading before its step: sfw_capi.hip prefix_classes::item_cols), items of a
  // SUFFIX / WHOLE launch are the chunk's samples.
  int32_t phase;                 // SFW_PHASE_*
  int32_t step_begin, step_end;  // steps this launch integrates
  int32_t resume;                // 1: start from in_state records instead of the initial agents
  int32_t force_alive;           // 1: K2 also integrates samples K1 rejected on the costmap (point dumps only)
  int32_t k2_form;               // SFW_K2_AUTO / _REGISTER / _FLAT: which organisation of a K2 wave (sfw_set_k2_form)
  int32_t n_cu, n_xcd;           // compute units / XCDs of the device (organisation thresholds, XCD-contiguous block order)
  int32_t n_cls, n_col_cls;      // PREFIX: classes of this level, its column classes
  // flat K2 only: the launch covers the items from item_base on (0: all of them) — a register-form launch may hand its last
  // items to flat-form waves (sfw_launch_social, sfw_split_streams)
  int32_t item_base;
  const int32_t *row_rep;        // PREFIX [row classes]  chunk-local row whose robot records represent the class
  const int32_t *col_rep;        // PREFIX [n_col_cls]    column likewise
  // where an item resumes from: record row_src[r] * n_col_src + col_src[c] of in_state, with (r, c) =
  // (row class, column class) of a PREFIX item, (chunk-local row, column) of a sample
  int32_t n_col_src;
  const int32_t *row_src, *col_src;
  const sfw_cls_agent *in_state;  // [source classes][A]
  const int32_t *in_dead;         // [source classes] 0, or 2 + step of a pedestrian contact so far
  sfw_cls_agent *out_state;       // PREFIX [n_cls][A]
  int32_t *out_dead;              // PREFIX [n_cls]
  // flat social kernel: pair u -> LDS plane byte offsets 8*i (first array) and 8*j (second array), padded with the
  // dummy slot 8*A; see sfw_launch_pair_table
  const uint16_t *pair_tab;
  // per-sample outputs, indexed by GLOBAL sample index
  int32_t *status;       // T
  double *base_cost;     // T : vel + distance + angle + costmap terms (ref :663-666)
  double *costs;         // T : final cost or sentinel
  int32_t *coll_step;    // T : step at which a pedestrian touched the robot (ref :613-627), -1 if none; nullable
  // per-chunk tables (see sfw_unit)
  sfw_unit *ptab;        // [step][row_units]: positions of the chunk's samples, then velocities of its grid rows
  sfw_unit *cs_tab;      // [step][nw]: cos / sin of the heading before the step, per grid column (a list: [step][rstep_stride])
  int64_t row_units;     // units per step row of ptab (>= rstep_stride + grid rows the chunk touches)
  int16_t *fcode;        // footprint cost per (step, sample): -3,-2,-1 or 0..253, [step][rstep_stride]
  int64_t rstep_stride;  // samples per step row (position units in a ptab row, codes in an fcode row)
  // optional Trajectory-points dump (x,y,theta per pre-step pose) of the chunk's samples
  double *points;        // nullable, chunk_count x S x 3 doubles
  int32_t *n_points;     // nullable, chunk_count ints
  // measurement only (sfw_set_timing): the middle block of a K2 launch leaves {s_memtime, s_memrealtime} at its start in [0..1]
  // and at its end in [2..3]; their ratio is the shader clock the kernel really ran at.  Nullable.
  unsigned long long *clock_probe;
  // one launch per control cycle (sfw_cycle_kernel): the selection's inputs and outputs ride with the scoring launch
  int64_t index_base;       // global iteration index of sample 0 (sfw_grid_stage)
  unsigned *cycle_counter;  // one word, zero between launches: blocks that have written their cost
  sfw_sel *sel_out;         // the selection record (device)
  double *costs_host;       // nullable: pinned mirror of the cost vector ...
  sfw_sel *sel_host;        // ... and of the record
  // sfw_cycle_kernel only, nullable: the stage's arena (footprint | agents | sample vectors | ...) has NOT been copied to the
  // device; every block copies it from the host's pinned memory to arena_dev itself, in front of everything else (all blocks
  // write the same bytes).  A control cycle whose costmap has not changed is then ONE kernel and no copy at all.
  const char *arena_host;
  char *arena_dev;
  uint32_t arena_bytes;
  // sfw_set_terms_capture, nullable: the five cost terms of every sample (SFW_TERM_*), SoA [SFW_N_TERMS][terms_T] by GLOBAL
  // sample index, written where base_cost / costs are (sfw_put_term*); a sentinel cost puts its sentinel into all five
  double *terms;
  int64_t terms_T;
  // sfw_samples_stage: the samples are a LIST, not a tensor product.  Sample t is the command (linvels[t], vy_samps[t] — 0.0
  // when vy_samps is null —, angvels[t]); nv = chunk rows = the list's length and nw = 1, so K2, the chunking and the ptab
  // addressing see a grid of n rows by one column (vel_row_of: one velocity unit per sample).  The list kernels (the *_list
  // instantiations of K1, the cycle kernel and the selection) never skip a sample and keep cs_tab as [step][rstep_stride]:
  // one cos / sin unit per sample of the chunk.  (Appended: no other field's offset moves.)
  const double *vy_samps;
  int32_t list;
  // sfw_sequences_stage: a list whose commands change inside the horizon.  linvels / vy_samps / angvels hold n_knots rows of
  // knot_stride (= the stage's sample count) values, knot-major: knot k of sample t at [k * knot_stride + t], so row 0 is where
  // a list's vectors lie (the selection and the re-score read it as they read a list's).  At step i the targets of
  // computeNewVelocity are those of the largest k with knot_step[k] <= i (knot_step[0] = 0, strictly ascending, read
  // wave-uniformly as the steps go by: no per-step table that sfw_set_params could leave stale).  n_knots <= 1: a plain list —
  // the list kernels run; n_knots > 1: the *_seq instantiations of K1 and of the cycle kernel, which write the list's table
  // layout.  (Appended: no other field's offset moves.)
  int32_t n_knots;
  const int32_t *knot_step;
  int64_t knot_stride;
  // sfw_set_footprint_clearance, nullable: one byte per costmap cell, 1 where every cell of the square window of half-width
  // r_c around the cell is on the map and has cost 0 — r_c so large that the window holds every cell a footprint check of a
  // pose in that cell can read (sfw_capi.hip clearance_half_width).  Such a pose's footprint cost is 0 without walking an edge
  // (sfw_kernels.hip footprint_cost_clear).  Null: every pose walks.  (Appended: no other field's offset moves.)
  const uint8_t *clear;
  // sfw_set_stop_check (stop_on: 0 off — nothing below is read and no kernel is added): the braking tail behind K1c
  // (sfw_kernels.hip sfw_stop_*_kernel).  stop_tail: [stop_cap][rstep_stride] frames (x, y, cos, sin) of the tail poses of the
  // chunk's samples, laid out like ptab / cs_tab (adjacent lanes store adjacent frames); stop_cap: the host's bound on the
  // tail length (sfw_capi.hip stop_tail_bound; a longer tail is still checked, serially, by the thread that walks it).
  // stop_steps / stop_hit: per sample, by GLOBAL sample index.  stop_points / stop_points_cap (nullable): the tail poses
  // (x, y, theta) of the chunk's samples, [chunk_count][stop_points_cap][3] (sfw_grid_stop_points).
  // (Appended: no other field's offset moves.)
  int32_t stop_on, stop_max_steps, stop_cap, stop_points_cap;
  double stop_dec_x, stop_dec_y, stop_dec_theta;
  sfw_pose_frame *stop_tail;
  int32_t *stop_steps, *stop_hit;
  double *stop_points;
  // sfw_set_path (path_on: 0 off — nothing below is read and no kernel is added): the path term behind K1c / the stop check
  // (sfw_kernels.hip sfw_path_*_kernel).  path_seg: path_n_seg segment records, read wave-uniformly; path_D: [step][rstep_stride]
  // squared distances of the chunk's poses, laid out like fcode; path_p: per sample, by GLOBAL sample index, the term or the
  // sample's sentinel.  (Appended: no other field's offset moves.)
  // path_slices: > 1 — the distance kernel's grid z: slices of 64 segments that meet by an integer atomicMin (a long path
  // under a launch that leaves the GPU idle); 0 or 1: one thread walks all segments of its pose
  int32_t path_on, path_n_seg, path_slices, path_pad;
  const sfw_path_seg *path_seg;
  double *path_D;
  double *path_p;
};

// cost + w * p behind the five-term sum: one product and one sum, each rounded once (the add kernel, the re-score kernel and
// the ensemble's aggregations share the statement)
__device__ __forceinline__ double sfw_cost_add_path(double cost, double w_path, double p) {
#pragma clang fp contract(off)
  return cost + w_path * p;
}

// Writers of the captured cost terms (no-ops when terms is null): term k of sample t, the three pedestrian-free terms, or one
// sentinel in all five
__device__ __forceinline__ void sfw_put_term(double *terms, int64_t T, int64_t t, int k, double v) {
  if (terms) terms[k * T + t] = v;
}
__device__ __forceinline__ void sfw_put_terms3(double *terms, int64_t T, int64_t t, double vel, double d, double ang) {
  if (!terms) return;
  terms[SFW_TERM_VEL * T + t] = vel;
  terms[SFW_TERM_DISTANCE * T + t] = d;
  terms[SFW_TERM_ANGLE * T + t] = ang;
}
__device__ __forceinline__ void sfw_put_terms_sentinel(double *terms, int64_t T, int64_t t, double sentinel) {
  if (!terms) return;
  for (int k = 0; k < SFW_N_TERMS; ++k) terms[k * T + t] = sentinel;
}


// sfw_score_one_crowd / sfw_grid_crowd: where sfw_crowd_kernel leaves the predicted crowd of its one sample.  Row i (step i)
// holds one entry per agent slot a (0 = the robot): the post-step state (x, y, vx, vy) — 32 bytes, 16-byte aligned —, the
// slot's work of the step and its goal flag.  A second kernel argument, not a part of sfw_launch: no other kernel's
// arguments change.
struct sfw_crowd_out {
  double *state;      // [S][A][4]
  double *work;       // [S][A]
  int32_t *has_goal;  // [S][A]
};

// Fills L.k from L.p and L.O (host).
void sfw_derive(sfw_launch &L);

// Launchers (sfw_kernels.hip).  All enqueue on `stream` and return hipError_t.
hipError_t sfw_launch_rollout(const sfw_launch &L, hipStream_t stream);  // = poses, then costmap
// The two halves of K1: the social kernel's prefix phase needs only the first (the robot-step
// table), so the second can run beside it on another stream.
hipError_t sfw_launch_rollout_poses(const sfw_launch &L, hipStream_t stream);
hipError_t sfw_launch_rollout_costmap(const sfw_launch &L, hipStream_t stream);
// sfw_set_path: costs[t] = costs[t] + w * p[t] for t in [begin, begin + count) where neither is a sentinel, behind K2 and in
// front of the selection (sfw_kernels.hip sfw_path_add_kernel; the distance and scan kernels ride with sfw_launch_rollout_costmap)
hipError_t sfw_launch_path_add(double *costs, const double *p, double w, int64_t begin, int64_t count, hipStream_t stream);
// The clearance map of a costmap (sfw_launch.clear): clear[c] = 1 iff the (2 r + 1)^2 window around cell c is on the map and
// all 0.  Two separable passes, rows into tmp (size_x * size_y bytes), then columns into clear.
hipError_t sfw_launch_clearance(const uint8_t *cells, uint32_t size_x, uint32_t size_y, int r, uint8_t *tmp, uint8_t *clear,
                                hipStream_t stream);
// sp (optional): a second stream and two events, with which a register-form launch whose waves do not divide evenly over
// the SIMDs hands its last items to concurrent flat-form waves (bit-identical organisations; sfw_kernels.hip split_point)
struct sfw_split_streams {
  hipStream_t side;
  hipEvent_t fork, join;
};
hipError_t sfw_launch_social(const sfw_launch &L, hipStream_t stream, const sfw_split_streams *sp = nullptr);
// K1 + K2 + K3 of a small grid in ONE launch (sfw_kernels.hip sfw_cycle_kernel); sfw_cycle_applies says whether a launch
// qualifies (L.cycle_counter / sel_out / index_base set; costs_host / sel_host optional)
bool sfw_cycle_applies(const sfw_launch &L);
hipError_t sfw_launch_cycle(const sfw_launch &L, hipStream_t stream);
// Many handles' control cycles in ONE launch (sfw_batch_*, sfw_kernels.hip sfw_batch_cycle_kernel).  The device table is
// first[B + 1] (uint32: member m owns blocks [first[m], first[m + 1]), one per sample) followed, at sfw_batch_recs_offset(B),
// by B records; the host fills it in pinned memory and copies it in one piece.  Members of one launch share the kernel
// instantiation: sfw_cycle_batch_variant is the grouping key, 9 * kind + 3 * precision + (groups / laser points / neither), with
// kind 0 a grid (sfw_batch_cycle_kernel: the values 0..8 grids have always had), 1 a sample list (sfw_batch_cycle_list_kernel),
// 2 sequences of more than one knot (sfw_batch_cycle_seq_kernel).
#define SFW_BATCH_VARIANTS 27
struct sfw_batch_rec {
  sfw_launch L;      // the member's launch as sfw_launch_cycle would launch it (sfw_cycle_batch_record)
  int32_t k2_bytes;  // its block's LDS layout: K2 wave's area | k1s_lds | cycle_result
  int32_t lds_bytes;
};
inline size_t sfw_batch_recs_offset(int B) { return (sizeof(uint32_t) * (static_cast<size_t>(B) + 1) + 15) & ~size_t(15); }
int sfw_cycle_batch_variant(const sfw_launch &L);
// rec <- L as the member of a batch (sfw_cycle_applies(L) must hold)
void sfw_cycle_batch_record(const sfw_launch &L, sfw_batch_rec *rec);
// one launch over `blocks` = first[B] blocks of `lds` dynamic LDS bytes each (the largest member's); every member of the
// table has the variant `variant`
hipError_t sfw_launch_cycle_batch(int variant, const uint32_t *d_first, const sfw_batch_rec *d_recs, int B, unsigned blocks,
                                  size_t lds, hipStream_t stream);
#ifndef SFW_STRICT_BUILD
hipError_t sfw_launch_cycle_batch_strict(int variant, const uint32_t *d_first, const sfw_batch_rec *d_recs, int B,
                                         unsigned blocks, size_t lds, hipStream_t stream);
// the same launcher over the K2 kernels compiled with the longer polynomials (sfw_kernels_strict.hip): SFW_PRECISION_F64_STRICT
// samples of a launch over T samples that the register form hands to flat-form waves (0: none)
int64_t sfw_social_flat_items(int A, int O, int NG, int64_t T, int form, int cus);
hipError_t sfw_launch_social_strict(const sfw_launch &L, hipStream_t stream, const sfw_split_streams *sp = nullptr);
hipError_t sfw_launch_cycle_strict(const sfw_launch &L, hipStream_t stream);
hipError_t sfw_launch_crowd_strict(const sfw_launch &L, const sfw_crowd_out &cw, hipStream_t stream);
#endif
// One wave integrates the ONE sample of L (chunk_count 1, whole rollout, K1 tables in place) with the crowd capture
// (sfw_kernels.hip sfw_crowd_kernel).  L.pair_tab must be a table built with runtime_cap (below); L.A >= 1.
hipError_t sfw_launch_crowd(const sfw_launch &L, const sfw_crowd_out &cw, hipStream_t stream);
// true when sfw_launch_rollout_poses runs all of K1 in one launch (small grids): the only form that writes L.points
// (of a launch over `count` samples of S steps)
bool sfw_rollout_is_fused(int64_t count, int S);
// Reduces costs[0..T) to one sfw_sel at *out (device memory).  partials must
// hold >= sfw_argmin_partials(T) records.
int64_t sfw_argmin_partials(int64_t T);
// costs_host / sel_host (nullable): host-visible pinned memory that receives a copy of the cost vector and of the record
// list: linvels / angvels hold one value per SAMPLE (sfw_launch.list), nw is not read
hipError_t sfw_launch_argmin(const double *costs, const double *linvels, const double *angvels,
                             int32_t nw, int64_t T, int64_t index_base, sfw_sel *partials,
                             sfw_sel *out, hipStream_t stream, double *costs_host = nullptr,
                             sfw_sel *sel_host = nullptr, bool list = false);
// sfw_grid_rescore: K weight vectors (device copy `w`) over the captured terms (SoA [5][T]) -> K records at sel_host (pinned).
// partials: K x sfw_rescore_blocks(T, K) records; costs (nullable): K x T doubles, weight-major.
int64_t sfw_rescore_blocks(int64_t T, int K);
hipError_t sfw_launch_rescore(const double *terms, int64_t T, const sfw_weights *w, int K, const double *linvels,
                              const double *angvels, int32_t nw, int64_t index_base, sfw_sel *partials, double *costs,
                              sfw_sel *sel_host, hipStream_t stream, bool list = false, const double *path_p = nullptr,
                              const double *path_w = nullptr);
// (path_p, nullable: the path term of the launch, sfw_launch.path_p; path_w: K path weights in device memory, read
// wave-uniformly — cost + path_w[k] * p behind the five-term sum where the cost is not a sentinel.  Null: the five terms alone.)
// sfw_ensemble_*: M members' captured terms (terms: device table of M pointers to SoA [5][T]; probs: M doubles, MEAN only —
// both read wave-uniformly) -> costs[T], rejected[T] (pinned or device) and the record at sel_host (pinned).  partials:
// sfw_argmin_partials(T) records.  One first stage of four, then the same second stage.
struct sfw_ensemble_launch {
  const double *const *terms;
  const double *probs;
  int M;
  int64_t T;
  int mode;
  sfw_weights w;
  // over a LIST the members staged (sfw_launch.list): linvels / angvels hold one value per sample (the first knot row), the
  // selection is the list's, no sample is skipped, nw is not read.  costs_dev (nullable, a list's only): a second,
  // device-resident copy of the cost vector.
  bool list;
  const double *linvels, *angvels;
  int32_t nw;
  double *costs, *costs_dev;
  int32_t *rejected;
  sfw_sel *partials, *sel_host;
  // under a risk (sfw_ensemble_set_risk; M <= SFW_ENSEMBLE_MAX_M): thr = contact_mass * P, the host's product
  bool risk;
  double tail_mass, contact_mass, thr;
  // path_p (nullable): member 0's path term — path_w * p[t] is added behind the aggregated five-term cost of a sample that is not
  // rejected, in front of the selection.  Null: the five terms alone.
  const double *path_p;
  double path_w;
};
hipError_t sfw_launch_ensemble(const sfw_ensemble_launch &a, hipStream_t stream);
// sfw_grid_blend: the cost vector (+ bias, nullable) of a launch over T samples -> softmin weights for L temperatures, their
// sums and the weighted mean of the K knot rows (list: linvels / vy (nullable) / angvels hold K rows of T values, knot-major;
// else a grid of T / nw x nw samples, K == 1).  Three launches: `mins` (sfw_blend_min_blocks(T) records), `partials`
// (sfw_blend_blocks(T) x sfw_blend_channels(L, K) doubles), then *min_host and out_host[sfw_blend_channels(L, K)] = eta[L] |
// sum_w2[L] | u[L][K][3] in pinned memory.  weights (nullable): L x T doubles, lambda-major.
// plan (nullable; sfw_mppi_run: L == 1, K x 3 doubles on the device): the last kernel is sfw_mppi_update_kernel — out_host
// receives eta | sum_w2 | the NEXT nominal plan, and `plan` becomes it: the blended knots, or unchanged when no sample is valid.
struct sfw_blend_min {
  double j;         // +inf when no sample is valid
  int64_t index;    // the largest t with J_t == j; -1
  int64_t n_valid;
};
struct sfw_blend_lambdas {
  double v[SFW_BLEND_MAX_L];
};
int64_t sfw_blend_blocks(int64_t T);
int64_t sfw_blend_min_blocks(int64_t T);
inline int64_t sfw_blend_channels(int L, int K) { return 2 * static_cast<int64_t>(L) + 3 * static_cast<int64_t>(K) * L; }
hipError_t sfw_launch_blend(const double *costs, const double *bias, int64_t T, const sfw_blend_lambdas &lam, int L, int K,
                            const double *linvels, const double *vy, const double *angvels, int32_t nw, bool list,
                            sfw_blend_min *mins, double *partials, double *weights, sfw_blend_min *min_host, double *out_host,
                            hipStream_t stream, double *plan = nullptr);
// The weights of L temperatures alone (a slice of a weights_out that does not fit one buffer), behind a sfw_launch_blend
// with the same costs and bias: `mins` as that launch left it.
hipError_t sfw_launch_blend_weights(const double *costs, const double *bias, int64_t T, const sfw_blend_lambdas &lam, int L,
                                    const sfw_blend_min *mins, double *weights, hipStream_t stream);
// sfw_sequences_perturb_stage: the K x n knot rows of a perturbed stage, drawn on the device (sfw_kernels.hip
// sfw_perturb_kernel).  vx / vy (nullable: SFW_PERTURB_NO_VY) / vtheta: K rows of n doubles, knot-major; z_out (nullable): the
// normals, [(k * 3 + c) * n + t].
struct sfw_perturb_dev {
  uint32_t key0, key1;  // the seed's low and high half
  int32_t keep_nominal, pad;
  double sigma[3], lo[3], hi[3];
  double nominal[SFW_SEQ_MAX_KNOTS * 3];  // [k][vx, vy, vtheta]; rows >= K are not read
};
hipError_t sfw_launch_perturb(const sfw_perturb_dev &a, int64_t n, int K, int64_t index_base, double *vx, double *vy, double *vtheta,
                              double *z_out, hipStream_t stream);
// sfw_perturb_dev up to the nominal rows: what a kernel that reads the plan from device memory takes as its argument
struct sfw_perturb_head {
  uint32_t key0, key1;
  int32_t keep_nominal, pad;
  double sigma[3], lo[3], hi[3];
};
static_assert(sizeof(sfw_perturb_head) == offsetof(sfw_perturb_dev, nominal), "sfw_perturb_head is the head of sfw_perturb_dev");
// The same draw around `plan` (K x 3 doubles in device memory; a.nominal is not read): sfw_perturb_plan_kernel
hipError_t sfw_launch_perturb_plan(const sfw_perturb_dev &a, const double *plan, int64_t n, int K, int64_t index_base, double *vx,
                                   double *vy, double *vtheta, double *z_out, hipStream_t stream);
// ... into the knot rows of M handles that stage the same sfw_perturb (sfw_ensemble_mppi_run), each value drawn once:
// sfw_perturb_members_kernel.  dst: M records in DEVICE memory; vy / z are null in every record or in none.
struct sfw_perturb_dst {
  double *vx, *vy, *vtheta, *z;
};
hipError_t sfw_launch_perturb_members(const sfw_perturb_dev &a, const double *plan, int64_t n, int K, int64_t index_base,
                                      const sfw_perturb_dst *dst, int M, hipStream_t stream);
// sfw_sequences_control_cost: bias[t] = gamma * c_t (+ bias_add[t], nullable) of the perturbed stage `a` describes, n doubles
// on the device.  plan (nullable): the nominal rows in device memory instead of a.nominal; z_kept (nullable): the stage's kept
// normals, else they are drawn again.
hipError_t sfw_launch_control_cost(const sfw_perturb_dev &a, const double *plan, int K, int64_t n, int64_t index_base,
                                   const double *z_kept, double gamma, const double *bias_add, double *bias, hipStream_t stream);
// Row r of the [R,5] multi-device exchange table from a selection record (+inf in every other row).
hipError_t sfw_launch_key_table(const sfw_sel *sel, double *table, int r, int R, hipStream_t stream);
// Pair table of the flat social kernel for A agents: sfw_pair_table_entries(A) uint16 entries.
int64_t sfw_pair_table_entries(int A);
// runtime_cap: the table of the kernel with run-time plane capacity whatever A is (sfw_crowd_kernel); the dummy slots differ
hipError_t sfw_launch_pair_table(uint16_t *tab, int A, hipStream_t stream, bool runtime_cap = false);
// Samples handled by one wave of the social kernel for A agents (form: SFW_K2_*).
// (cus: compute units of the device, sfw_launch.n_cu)
int sfw_samples_per_wave(int A, int64_t T, int form, int cus);
size_t sfw_social_lds_bytes(int A, int O, int NG, int n_grp_mem, int64_t T, int form, int cus);
// SFW_ORG_* of a K2 launch over T items
int sfw_social_organisation(int A, int64_t T, int O, int form, int cus);

#endif  // SFW_DEVICE_H_
