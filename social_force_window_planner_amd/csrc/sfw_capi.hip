// sfw_capi.hip — host side of the C ABI declared in include/sfw_hip.h.
// Owns the device buffers, the handle's HIP stream and events, and sequences
// the three kernels of sfw_kernels.hip.  There is NO CPU fallback: without a
// HIP device sfw_create fails with SFW_ERR_NO_DEVICE.

#include "sfw_device.h"

#include <dlfcn.h>
#include <link.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

namespace {

// Owning buffers: not copyable, so that nothing holding one by value can free it twice.
template <typename T> struct dev_buf {
  T *p = nullptr;
  size_t cap = 0;  // elements
  dev_buf() = default;
  dev_buf(const dev_buf &) = delete;
  dev_buf &operator=(const dev_buf &) = delete;
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = n + n / 8 + 16;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), want * sizeof(T));
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// ---- the footprint clearance map (sfw_launch.clear, sfw_set_footprint_clearance) ----
// A window of more than 2 * kClearMaxHalfWidth + 1 = 129 cells: no map, every pose walks (a footprint of 3 m at 0.05 m per
// cell; the build's cost grows with the window and a window that wide is clear almost nowhere)
constexpr int kClearMaxHalfWidth = 64;
// Poses (samples x steps) of a stage from which it builds the map: 96 x 96 samples at 40 steps, the smallest grid measured at
// which a build before EVERY step (a costmap that changes every cycle) still left the step shorter than walking every pose
// (+5..+7 us at 9 216 samples; -6..-12 us at 4 096, where an unchanged map gained 1..4 us; control cycles never get here).
// profiles/r23_footprint_clearance.txt has the sweep.
constexpr int64_t kClearMinPoses = 368640;

// Pinned host staging area for one logical upload.  The caller's buffer is copied
// here synchronously (so it may be freed or reused on return) and the H2D copy is
// enqueued on the handle's stream; `done` guards the area against being rewritten
// while that copy is still pending.  No stream synchronisation on the hot path.
struct pinned_buf {
  char *p = nullptr;
  size_t cap = 0;
  hipEvent_t done = nullptr;
  bool pending = false;
  pinned_buf() = default;
  pinned_buf(const pinned_buf &) = delete;
  pinned_buf &operator=(const pinned_buf &) = delete;
  hipError_t wait() {
    if (!pending) return hipSuccess;
    pending = false;
    return hipEventSynchronize(done);
  }
  hipError_t reserve(size_t bytes) {
    hipError_t e = wait();
    if (e != hipSuccess) return e;
    if (!done && (e = hipEventCreateWithFlags(&done, hipEventDisableTiming)) != hipSuccess) return e;
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    const size_t want = bytes + bytes / 4 + 256;
    e = hipHostMalloc(reinterpret_cast<void **>(&p), want, hipHostMallocDefault);
    if (e == hipSuccess) cap = want;
    return e;
  }
  hipError_t mark(hipStream_t s) {
    pending = true;
    return hipEventRecord(done, s);
  }
  void release() {
    (void)wait();
    if (p) (void)hipHostFree(p);
    if (done) (void)hipEventDestroy(done);
    p = nullptr;
    cap = 0;
    done = nullptr;
  }
};

// shared-prefix plan of the staged grid (sfw_device.h: sfw_cls_agent): per chunk of whole rows, the class tables of each level
struct level_tables {               // offsets (ints) into the plan's class tables
  int32_t n_row = 0, n_col = 0;     // classes of the level: rows in this chunk x columns
  size_t o_row_rep = 0, o_col_rep = 0;  // representative chunk-local row / column of a class
  size_t o_row_src = 0, o_col_src = 0;  // class of the previous level a class resumes from (level > 0)
};
struct chunk_plan {
  std::vector<level_tables> lv;
  size_t o_row_cls = 0;             // chunk-local row -> row class of the last level
};

struct map_geometry {
  uint32_t size_x, size_y;
  double origin_x, origin_y, resolution;
};

// An agent set as sfw_set_agents packs it (uploaded with the next stage).  A value: sfw_multi_set_agents copies rank 0's.
struct agent_set {
  std::vector<char> blob;  // pos | vel | const | obstacles | grp | off | mem, 16-byte aligned parts
  size_t ao_vel = 0, ao_cst = 0, ao_obs = 0, ao_grp = 0, ao_off = 0, ao_mem = 0;
  int A = 0, O = 0, NG = 0, n_grp_mem = 0;
  bool person_pinned = false;  // some person i >= 1 can never move (desired_velocity == 0): see rest_noise_unreproduced
  // ordered pairs (i, j) of agents with w x diff == 0 at hand-over (standing people, collinear walkers): see rest_forces
  std::vector<std::pair<int32_t, int32_t>> rest_pairs;
};

// The buffers of a softmin blend, one set per owner (a handle's sfw_grid_blend; an sfw_ensemble's sfw_ensemble_blend, which
// runs on member 0's stream but must not touch what belongs to that member's own calls): first-pass records, per-block partial
// sums, the bias and weight vectors on the device; pin receives the minimum record | eta[L] | sum_w2[L] | u[L][K][3] from the
// kernels
struct blend_buffers {
  dev_buf<sfw_blend_min> mins;
  dev_buf<double> partials, bias, weights;
  pinned_buf pin;
  void release() {
    mins.release();
    partials.release();
    bias.release();
    weights.release();
    pin.release();
  }
};
// ... and of the control cost and the MPPI chain: the bias vector gamma * c_t (+ bias_t) on the device; the nominal plan on the
// device (SFW_SEQ_MAX_KNOTS x 3 doubles, moved on by every iteration's update kernel); pin_mppi = one blend slot per iteration |
// the caller's nominal (the source of the copy that starts the chain) [| an ensemble's member table: ensemble_mppi_chain]
struct mppi_buffers {
  dev_buf<double> ctrl_bias, mppi_plan;
  pinned_buf pin_mppi;
  void release() {
    ctrl_bias.release();
    mppi_plan.release();
    pin_mppi.release();
  }
};

// The scratch outputs of a re-run of some samples of the staged grid (sfw_grid_points_batch, sfw_grid_stop_points, crowd_run:
// reserve_scratch, fill_scratch_launch), so that the launch's own results stay intact: one set per handle, kept across calls
// (hipMalloc/hipFree synchronise the device) — per-sample records, the K1 tables, the stop check's records and tail table, the
// path term's distance table and term
struct rerun_buffers {
  dev_buf<int32_t> status, coll, stop_steps, stop_hit;
  dev_buf<double> base, costs, path_D, path_p;
  dev_buf<sfw_unit> ptab, cs;
  dev_buf<int16_t> fcode;
  dev_buf<sfw_pose_frame> stop_tail;
  void release() {
    status.release();
    coll.release();
    stop_steps.release();
    stop_hit.release();
    base.release();
    costs.release();
    path_D.release();
    path_p.release();
    ptab.release();
    cs.release();
    fcode.release();
    stop_tail.release();
  }
};

}  // namespace

// The handle's state, grouped by who owns it:
//   cfg    fixed by sfw_create (and its environment);
//   live   switches sfw_set_* change at any time, read by every stage and launch;
//   world  what sfw_set_costmap / _footprint / _agents hold on the host until the next stage;
//   st     what the last stage recorded and uploaded: a launch, sfw_grid_plan_info and the points dump read this, never `world`;
//   last   what the last launch did: fetch, views and the per-launch queries read this.
// A stage past its argument checks drops `st` and `last` first and sets st.valid last; a launch drops `last` first and sets
// last.launched last.  A call that fails in between leaves nothing staged (or launched), never a mix of two calls.
struct sfw_planner_s {
  struct config {
    // shape of the device the launch heuristics are scaled to: compute units (hipDeviceProp_t.multiProcessorCount: 256 on a
    // whole MI355X, 32 on a CPX partition) and XCDs (32 CUs each); SFW_DEVICE_CUS / SFW_DEVICE_XCDS in the environment of
    // sfw_create override them (a test pretends 32 CUs: the plan changes, the results may not)
    int n_cu = SFW_DEFAULT_CUS, n_xcd = SFW_DEFAULT_CUS / SFW_CUS_PER_XCD;
    std::vector<int> prefix_env;  // SFW_PREFIX: empty automatic, {0} off, else forced split steps
    bool pin_rest_on = true;      // SFW_PIN_REST=0: no pinned-rest table (tests: what it changes)
    long spin_us = 20000;         // SFW_SPIN_US: how long a fetch polls the stream before it blocks in hipStreamSynchronize
                                  // (0: block at once)
    bool arena_direct_on = true;  // SFW_ARENA_DIRECT=0: always copy the arena at stage time
    size_t mirror_max_bytes = size_t(64) << 20;  // SFW_MIRROR_MAX_MB; 0: always copy
    int obs_tasks_force = -1;     // SFW_OBS_TASKS=0|1: the flat form's laser-point pass as one lane per agent / as (agent,
                                  // segment) tasks, whatever sfw_derive prices (tuning aid)
    size_t table_budget_bytes = size_t(8) << 30;  // K1->K2 per-step tables per chunk (of 288 GB): BASELINE cfg4 runs in one chunk
    // a member of a sfw_batch: the batch's streams are borrowed (sfw_destroy refuses the handle; the batch destroys it)
    bool owns_streams = true;
    bool batch_member = false;
    // poses (samples x steps) of a stage from which it builds the footprint clearance map when there is none for its costmap
    // and footprint (kClearMinPoses has the measurement); SFW_CLEAR_MIN_POSES overrides it (0: every stage builds — tests)
    int64_t clear_min_poses = kClearMinPoses;
    // SFW_STOP_TABLE_ROWS (tests): at most this many rows in the stop check's tail table, whatever stop_tail_bound says — the
    // tail steps beyond them are checked by the thread that walks the tail (sfw_stop_tail_kernel), with the same result
    int stop_rows_max = -1;
    // SFW_PATH_SLICES=0 (A/B and tests): the path term's distance kernel never splits the segments over the grid's z
    bool path_slices_on = true;
  } cfg;

  struct switches {
    sfw_params params;
    uint64_t params_epoch = 1;  // bumped by sfw_set_params; st.plan_epoch says which epoch the stage's plan was made for
    int k2_form = SFW_K2_AUTO;  // sfw_set_k2_form / SFW_FORCE_FLAT
    bool timing = false;        // sfw_set_timing: record the per-kernel events sfw_last_launch_ms reads
    // sfw_set_points_capture: a grid small enough for the fused K1 (a control cycle's samples) leaves its Trajectory points,
    // point counts and contact steps during the scoring launch itself, in one buffer (pin_cap) -> the dump is one memcpy
    bool capture_points = false;
    // sfw_set_terms_capture: every grid launch also leaves the five cost terms of every sample in `terms` (SoA [5][T])
    bool capture_terms = false;
    // sfw_set_footprint_clearance: K1b reads the clearance map of a stage that has one (off: every pose walks its edges)
    bool fp_clear = true;
    // sfw_set_stop_check: the braking tail behind the costmap scan (off: no kernel is added); read by the next stage
    bool stop_on = false;
    sfw_stop_check stop{};
    // sfw_set_path: the path term (off: no kernel is added); read by the next stage.  path_xy: the points as handed over
    bool path_on = false;
    double path_weight = 0.0;
    std::vector<double> path_xy;
  } live;

  // Footprint, agents and laser points are small: sfw_set_* keep them on the host and every stage packs them into ONE
  // pinned arena and issues ONE H2D copy into `arena` — a control cycle is latency-bound and each separate copy costs as
  // much as a kernel launch.  The costmap's cells wait in pin_map.
  struct world_state {
    map_geometry map_new{0, 0, 0, 0, 0};  // what sfw_set_costmap handed over last (pin_map holds its cells)
    bool have_costmap = false;
    bool cells_dirty = false;             // ... and the device has not seen yet
    uint64_t cells_gen = 0;               // bumped whenever sfw_set_costmap takes a snapshot that differs from the last
    std::vector<double> footprint;        // 2K
    int K = 0;
    agent_set agents;
  } world;

  struct stage_record {
    bool valid = false;  // everything below describes what the device holds; false: nothing is staged
    // the grid
    std::vector<double> lin, ang;
    int nv = 0, nw = 0;
    sfw_robot_state rs{};
    sfw_goal_args ga{};
    double vy_samp = 0.0;
    int skip_zero = 1;
    int64_t index_base = 0;
    // sfw_samples_stage: a LIST of nv samples (nw = 1).  lin / ang hold vx / vtheta of every sample, vy its vy (empty: all 0.0);
    // no shared-prefix plan is made, and the cos / sin table holds a unit per sample of a chunk (sfw_device.h sfw_launch.list)
    bool list = false;
    std::vector<double> vy;
    // sfw_sequences_stage: a list whose commands change inside the horizon.  lin / vy / ang then hold nk rows of nv values,
    // knot-major (row 0 = the first knot: what a list's vectors are to the selection and to sel_to_best); knot_step the nk
    // steps at which a knot takes over.  nk == 1: a plain list.
    int nk = 1;
    std::vector<int32_t> knot_step;
    const int32_t *d_knot_step = nullptr;
    // sfw_sequences_perturb_stage: the knot rows were drawn on the device (sfw_perturb_kernel) — lin / vy / ang stay EMPTY, the
    // arena's knot regions are never filled or sent from the host, and such a stage is never left arena_pending.  zero_admitted:
    // the clamp box admits a zero translation command (rest_noise_unreproduced); normals_kept: `normals` holds 3 nk nv doubles
    bool perturbed = false, zero_admitted = false, normals_kept = false;
    // ... and what they were drawn from (seed, sigma, box, KEEP_NOMINAL, the nominal rows), for sfw_sequences_control_cost.
    // Host memory only: the stage pays a struct copy for it
    sfw_perturb_dev pert{};
    // the world as uploaded (sfw_set_* after a stage take effect at the next stage; a launch in between must keep
    // describing the device copy)
    int K = 0, A = 0, O = 0, NG = 0, n_grp_mem = 0;
    bool person_pinned = false;       // (agent_set)
    map_geometry map{0, 0, 0, 0, 0};
    const uint8_t *d_cells = nullptr;
    bool cells_in_arena = false;      // the device copy of the cells is the head of `arena` (small maps), else `cells`
    size_t arena_cells_bytes = 0;     // bytes of that head
    // device pointers: offsets into `arena`, except d_sel (behind the cost vector in `costs`)
    const double *d_footprint = nullptr, *d_agent_pos = nullptr, *d_agent_vel = nullptr, *d_obstacles = nullptr;
    const sfw_agent_const *d_agent_c = nullptr;
    const int32_t *d_agent_grp = nullptr, *d_grp_off = nullptr, *d_grp_mem = nullptr;
    const double *d_linvels = nullptr, *d_angvels = nullptr;
    const double *d_vy = nullptr;          // the list's vy vector, or null (a grid; a list without one)
    const double *d_agent_rest = nullptr;  // A x (fx, fy), or null when there is no pair at relative rest
    const double *d_pin_rest = nullptr;    // see pinned_rest_table: the stage's table, or null
    sfw_sel *d_sel = nullptr;
    // what the relative-rest terms and the pinned-rest table were built from (sfw_set_params between stage and launch
    // rebuilds them)
    std::vector<std::pair<int32_t, int32_t>> rest_pairs;
    std::vector<double> rest_pv;      // pos | vel, 4A doubles
    size_t pin_doubles = 0;           // the pinned-rest table's length (4 + A) when the stage built one
    std::vector<double> pin_pos;
    std::vector<sfw_agent_const> pin_cst;
    // the shared-prefix plan (no levels: not used) and the K1->K2 table size, made for params epoch plan_epoch
    std::vector<int> prefix_steps;    // P(0) < P(1) < ...: level l integrates steps [P(l-1), P(l))
    std::vector<chunk_plan> prefix_chunks;
    size_t prefix_o_col_cls = 0;      // column -> column class of the last level
    int prefix_S = 0;
    int64_t prefix_chunk = 0;
    int64_t prefix_class_steps = 0, prefix_last_classes = 0;
    std::vector<int32_t> cls_ints;    // the plan's class tables as planned on the host (level_tables offsets index it)
    int64_t cls_max = 0;              // largest class count of a level (sizes cls_state / cls_dead)
    bool cls_two = false;             // more than one level: both ping-pong buffers
    const int32_t *d_cls_tab = nullptr;  // ... on the device: inside `arena` (staged with it) or d_cls (re-planned at launch)
    int64_t table_chunk = 0;          // samples per chunk the K1 tables hold
    uint64_t plan_epoch = 0;
    // the arena left in pin_arena only, for the launch's kernel to fetch (see stage_common / flush_arena)
    bool arena_pending = false;
    size_t arena_from = 0, arena_bytes = 0;
    // K1a of a single-chunk grid is enqueued by the STAGE, before the shared-prefix planning (25..45 us of host work that
    // the pose rollout does not depend on): early_poses says the staged grid's robot-step table is already in the stream
    bool early_poses = false;
    bool early_poses_timed = false;  // ... and the stage recorded ev[0] in front of it (timing was on at stage time)
    bool early_poses_terms = false;  // ... and it wrote the pedestrian-free terms too
    bool clock_cleared = false;      // the stage cleared the clock probe in front of the pose rollout it started
    // the footprint clearance map (stage_clearance): clear_map describes the staged costmap and footprint, for windows of
    // half-width clear_r cells (-1: the footprint is too large for a map)
    bool clear_on = false;
    int clear_r = -1;
    // the stop check as the stage found it (sfw_set_stop_check after a stage takes effect at the next stage), and the rows of
    // the tail table: the host's bound on the tail length (stop_tail_bound), made with the plan for params epoch plan_epoch
    bool stop_on = false;
    sfw_stop_check stop{};
    int stop_cap = 0;
    // the path term as the stage found it (sfw_set_path after a stage takes effect at the next stage): the segment records
    // (path_segments) that `path_seg` on the device holds for this stage, and the weight
    bool path_on = false;
    double path_weight = 0.0;
    std::vector<sfw_path_seg> path_segs;
  } st;

  // What `clear_map` on the device was built from (valid: it is enqueued or done): the snapshot's generation, the map's
  // size and the window's half-width.  A stage builds again when any of them differs from its own.
  struct clearance_record {
    bool valid = false;
    uint64_t cells_gen = 0;
    uint32_t size_x = 0, size_y = 0;
    int r = 0;
  } clr;

  struct launch_record {
    bool launched = false;  // every kernel of the launch is enqueued; false: nothing to fetch
    bool timed = false;     // ... with the per-kernel events (sfw_last_launch_ms)
    bool cycle = false;     // ... as the one-kernel control cycle
    bool fetched = false;   // a fetch has waited for it (sfw_grid_costs_view)
    bool mirrored = false;  // its selection kernels left costs + record in pin_mirror (sfw_launch_argmin)
    bool captured = false;  // it left Trajectory points in pin_cap (sfw_set_points_capture) ...
    int cap_S = 0;          // ... for this step count (the dump's layout)
    bool terms = false;     // it left the cost terms in `terms` (sfw_grid_rescore / sfw_grid_terms)
    int n_chunks = 1;
  } last;
  uint64_t launch_seq = 0;  // grid launches so far, never reset (an sfw_ensemble tells its own launch from a member's later one)

  // device, streams, events
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t side = nullptr;  // K1b + K1c beside the shared-prefix phase of K2
  hipEvent_t ev_poses = nullptr, ev_side = nullptr;
  // the samples' K2 launch may hand its last items to flat-form waves on `side` (sfw_launch_social, sfw_split_streams)
  sfw_split_streams split{nullptr, nullptr, nullptr};
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  std::vector<hipEvent_t> chunk_ev;  // 3 per chunk of a multi-chunk launch: K1 start, K1 end/K2 start, K2 end
  std::string err;
  const void *shared_cols = nullptr;  // axis_classes of the angular targets lent by sfw_multi_score_grid for the stage in
                                      // progress (every rank has the same column axis), else null

  // owned buffers
  dev_buf<uint8_t> cells;      // the costmap on the device when it is too large to ride in `arena`
  dev_buf<char> arena;         // the stage's one H2D copy: [cells] | footprint | agents | sample vectors | rest | class tables
  dev_buf<uint16_t> pair_tab;  // rebuilt when the agent count changes
  int pair_tab_A = -1;         // ... for this many agents (-1: none)
  dev_buf<unsigned> cycle_counter;  // the one-kernel control cycle's "blocks done" word (zero between launches)
  dev_buf<int32_t> d_cls, cls_dead[2];
  dev_buf<sfw_cls_agent> cls_state[2];  // ping-pong between levels
  // per-sample outputs + per-chunk table
  dev_buf<int32_t> status, coll_step;
  dev_buf<double> base_cost, costs;  // costs: T doubles followed by the sfw_sel record (one D2H fetches both)
  dev_buf<sfw_unit> ptab, cs_tab;   // the K1 tables (sfw_device.h sfw_unit), sized for st.table_chunk samples per step row
  dev_buf<int16_t> fcode;
  dev_buf<uint8_t> clear_map, clear_tmp;  // the footprint clearance map and the row pass's intermediate (one byte per cell each)
  dev_buf<sfw_sel> partials;
  dev_buf<double> points;
  dev_buf<int32_t> n_points;
  dev_buf<unsigned long long> clock;  // sfw_launch.clock_probe (timing only)
  dev_buf<char> one_out;  // sfw_score_one: cost | n_points | coll_step | points, contiguous -> one D2H
  rerun_buffers pts;  // the scratch outputs of the re-runs
  // the stop check's tail: per-sample records (T) and the per-chunk frame table (st.stop_cap rows of st.table_chunk frames);
  // the poses sfw_grid_stop_points reads back
  dev_buf<int32_t> stop_steps, stop_hit;
  dev_buf<sfw_pose_frame> stop_tail;
  dev_buf<double> stop_pts;
  // the path term: the stage's segment records (path_seg_sent: what the device copy holds, or is about to), the per-chunk
  // distance table [S][st.table_chunk] and the term per sample (T)
  dev_buf<sfw_path_seg> path_seg;
  pinned_buf pin_path;  // the records on their way to path_seg
  std::vector<sfw_path_seg> path_seg_sent;
  dev_buf<double> path_D, path_p, rescore_pw;
  pinned_buf pin_map, pin_arena, pin_out, pin_cls;
  pinned_buf pin_one;     // sfw_score_one's outputs where the one-launch kernel writes them (cost | n_points | coll_step | points)
  pinned_buf pin_mirror;  // costs + selection record as the selection kernels of the last launch leave them (device writes)
  pinned_buf pin_cap;     // points (24 S T bytes) | n_points (4 T) | contact steps (4 T), written by a capturing launch
  dev_buf<double> terms;  // the cost terms of a capturing launch (allocated by the first, freed by sfw_set_terms_capture(h, 0))
  dev_buf<sfw_weights> rescore_w;  // sfw_grid_rescore: the weight vectors on the device, its partial records, its cost vectors
  dev_buf<sfw_sel> rescore_partials;
  dev_buf<double> rescore_costs;
  pinned_buf pin_rescore;          // K records (written by the kernels) | K weight vectors (copied from)
  blend_buffers blend;  // sfw_grid_blend / sfw_grid_blend_control
  mppi_buffers mppi;    // sfw_sequences_control_cost / sfw_grid_blend_control (ctrl_bias), sfw_mppi_run
  // sfw_sequences_perturb_stage: the normals of a stage with SFW_PERTURB_KEEP_NORMALS; pin_knots receives the winner's first knot
  // (sel_to_best) and the ranges sfw_sequences_knots / _normals read back
  dev_buf<double> normals;
  pinned_buf pin_knots;
  // sfw_score_one_crowd / sfw_grid_crowd: cost | n_points | coll_step | state [S][A][4] | work [S][A] | has_goal [S][A],
  // contiguous -> one D2H into pin_crowd; the pair table of the kernel with run-time plane capacity (sfw_crowd_kernel)
  dev_buf<char> crowd_out;
  pinned_buf pin_crowd;
  dev_buf<uint16_t> crowd_pair_tab;
  int crowd_pair_tab_A = -1;
};

namespace {

int fail(sfw_handle h, int code, const std::string &msg) {
  if (h) h->err = msg;
  return code;
}
int hip_fail(sfw_handle h, hipError_t e, const char *what) {
  return fail(h, SFW_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define SFW_HIP(h, call)                                   \
  do {                                                     \
    hipError_t e_ = (call);                                \
    if (e_ != hipSuccess) return hip_fail((h), e_, #call); \
  } while (0)

// A stage past its argument checks, and a launch past its "nothing staged" check, first forget what the last one recorded:
// a failure from there on leaves nothing staged (or launched), never a record that mixes two calls.
void drop_launch(sfw_handle h) { h->last = sfw_planner_s::launch_record{}; }
void drop_stage(sfw_handle h) {
  h->st.valid = false;
  h->st.arena_pending = false;
  h->st.early_poses = false;
  drop_launch(h);
}

// K2 through the kernels the precision mode names (SFW_PRECISION_F64_STRICT: the build with the longer polynomials)
hipError_t launch_social_of(const sfw_launch &L, hipStream_t stream, const sfw_split_streams *sp = nullptr) {
  return L.p.precision == SFW_PRECISION_F64_STRICT ? sfw_launch_social_strict(L, stream, sp) : sfw_launch_social(L, stream, sp);
}

// SFW_DEVICE_CUS in the environment: pretend a device of that many compute units (planning heuristics only)
int env_device_cus(int fallback) {
  if (const char *b = std::getenv("SFW_DEVICE_CUS")) {
    const long v = std::atol(b);
    if (v >= 1 && v <= 4096) return static_cast<int>(v);
  }
  return fallback;
}

bool all_finite(const double *v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// Wait for the handle's stream.  hipStreamSynchronize parks the thread on an interrupt once its short active wait is over,
// and waking up costs 10-20 us — of a 100 us control cycle or a 600 us grid; the blocking call polls the stream instead
// (one core busy for the duration of the launch, as a caller asking hipDeviceScheduleSpin would have it) for up to spin_us,
// then blocks.
hipError_t poll_stream(sfw_handle h) {
  if (h->cfg.spin_us > 0) {
    const auto t0 = std::chrono::steady_clock::now();
    bool polled = false;
    for (;;) {
      const hipError_t e = hipStreamQuery(h->stream);
      if (e != hipErrorNotReady) {
        // ("not ready" is an answer, not an error: a runtime that records it as the thread's last error must not hand it to the
        // next launch's hipGetLastError)
        if (polled && e == hipSuccess) (void)hipGetLastError();
        return e;
      }
      polled = true;
      if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > h->cfg.spin_us) break;
#if defined(__x86_64__)
      __builtin_ia32_pause();
#endif
    }
    (void)hipGetLastError();
  }
  return hipStreamSynchronize(h->stream);
}
// ... after which no upload enqueued on it is still reading its pinned staging area
void stream_is_idle(sfw_handle h) { h->pin_map.pending = h->pin_arena.pending = h->pin_cls.pending = false; }
hipError_t wait_stream(sfw_handle h) {
  const hipError_t e = poll_stream(h);
  if (e == hipSuccess) stream_is_idle(h);
  return e;
}

// the register-form K2 addresses a unit inside a step row of the position / velocity table by a 32-bit byte offset: a row of
// `chunk` positions and at most chunk + 2 velocities (a one-column grid) must stay below 4 GB
constexpr int64_t kRowLimit = static_cast<int64_t>((uint64_t(1) << 32) / (2 * sizeof(sfw_unit))) - 2;

// (of params check_params has admitted: the quotient is finite and below SFW_MAX_STEPS + 1, so the conversion is defined)
int num_steps_of(const sfw_params &p) {
  int n = static_cast<int>(p.sim_time / p.sim_granularity + 0.5);  // ref :519
  return n == 0 ? 1 : n;                                           // ref :523-525
}

int check_params(sfw_handle h, const sfw_params *p) {
  if (!p) return fail(h, SFW_ERR_INVALID_ARG, "params is NULL");
  if (!(p->sim_granularity > 0) || !(p->sim_time >= 0))
    return fail(h, SFW_ERR_INVALID_ARG, "sim_time/sim_granularity out of range");
  // The step count sizes every table and is an `int` everywhere: a quotient that does not fit has no defined conversion
  // (sfw_hip.h SFW_MAX_STEPS).  The compare is written so that an infinite or NaN quotient fails it.
  if (!std::isfinite(p->sim_time) || !std::isfinite(p->sim_granularity) ||
      !(p->sim_time / p->sim_granularity + 0.5 < static_cast<double>(SFW_MAX_STEPS) + 1.0))
    return fail(h, SFW_ERR_INVALID_ARG, "sim_time/sim_granularity not finite, or more than SFW_MAX_STEPS steps");
  // the velocity term divides by max_vel_x (ref :654): 0 gives 0/0 or x/0, a cost that is neither a cost nor a sentinel
  if (!std::isfinite(p->max_vel_x) || p->max_vel_x == 0.0)
    return fail(h, SFW_ERR_INVALID_ARG, "max_vel_x must be finite and not 0");
  if (p->precision != SFW_PRECISION_F64 && p->precision != SFW_PRECISION_F32 && p->precision != SFW_PRECISION_F64_STRICT)
    return fail(h, SFW_ERR_INVALID_ARG, "unknown precision");
  if (!(p->sfm_gamma > 0) || !(p->sfm_relaxation_time > 0) || !(p->sfm_force_sigma_obstacle > 0))
    return fail(h, SFW_ERR_INVALID_ARG, "sfm gamma/relaxation_time/sigma must be > 0");
  if (!(p->sfm_force_factor_social >= 0) || !(p->sfm_force_factor_obstacle >= 0))
    return fail(h, SFW_ERR_INVALID_ARG, "sfm_force_factor_social / _obstacle must be >= 0");
  return SFW_OK;
}

// Units per step row of the position / velocity table for chunks of `stride` samples of an nw-column grid: the positions,
// then one velocity unit per grid row a chunk can touch (it may begin and end inside a row)
int64_t table_row_units(int64_t stride, int nw) { return stride + stride / (nw > 0 ? nw : 1) + 2; }
// bytes of the K1 tables per sample and step (position unit + footprint code; the per-row / per-column units are noise)
constexpr size_t kTableBytesPerSampleStep = sizeof(sfw_unit) + sizeof(int16_t);

// Fill the launch descriptor for samples [begin, begin+count).
void fill_launch(sfw_handle h, sfw_launch &L, int64_t begin, int64_t count, int64_t stride) {
  std::memset(&L, 0, sizeof(L));
  L.p = h->live.params;
  L.S = num_steps_of(h->live.params);
  L.dt = h->live.params.sim_time / L.S;  // ref :527
  L.rs = h->st.rs;
  L.ga = h->st.ga;
  L.vy_samp = h->st.vy_samp;
  L.skip_zero_sample = h->st.skip_zero;
  L.linvels = h->st.d_linvels;
  L.angvels = h->st.d_angvels;
  L.nv = h->st.nv;
  L.nw = h->st.nw;
  L.vy_samps = h->st.d_vy;
  L.list = h->st.list ? 1 : 0;
  L.n_knots = h->st.nk;
  L.knot_step = h->st.d_knot_step;
  L.knot_stride = h->st.nv;  // (a chunk's knot rows are addressed with the whole stage's stride: the kernels index them by the global sample)
  L.chunk_begin = begin;
  L.chunk_count = count;
  L.cells = h->st.d_cells;
  L.size_x = h->st.map.size_x;
  L.size_y = h->st.map.size_y;
  L.origin_x = h->st.map.origin_x;
  L.origin_y = h->st.map.origin_y;
  L.resolution = h->st.map.resolution;
  L.footprint = h->st.d_footprint;
  L.K = h->st.K;
  L.clear = (h->live.fp_clear && h->st.clear_on) ? h->clear_map.p : nullptr;
  L.agent_pos = h->st.d_agent_pos;
  L.agent_vel = h->st.d_agent_vel;
  L.agent_c = h->st.d_agent_c;
  L.agent_rest = h->st.d_agent_rest;
  L.pin_rest = h->st.d_pin_rest;
  L.A = h->st.A;
  L.obstacles = h->st.d_obstacles;
  L.O = h->st.O;
  L.agent_grp = h->st.d_agent_grp;
  L.grp_off = h->st.d_grp_off;
  L.grp_mem = h->st.d_grp_mem;
  L.NG = h->st.NG;
  L.n_grp_mem = h->st.n_grp_mem;
  L.n_cu = h->cfg.n_cu;
  L.n_xcd = h->cfg.n_xcd;
  sfw_derive(L);
  if (h->cfg.obs_tasks_force >= 0 && L.O > 0) L.k.obs_tasks = h->cfg.obs_tasks_force;
  L.pair_tab = h->pair_tab.p;
  L.status = h->status.p;
  L.base_cost = h->base_cost.p;
  L.costs = h->costs.p;
  L.coll_step = h->coll_step.p;
  L.ptab = h->ptab.p;
  L.cs_tab = h->cs_tab.p;
  L.row_units = table_row_units(stride, h->st.nw);
  L.fcode = h->fcode.p;
  L.rstep_stride = stride;
  L.points = nullptr;
  L.n_points = nullptr;
  L.phase = SFW_PHASE_WHOLE;
  L.step_begin = 0;
  L.step_end = L.S;
  L.resume = 0;
  L.k2_form = h->live.k2_form;
  L.index_base = h->st.index_base;
  L.cycle_counter = h->cycle_counter.p;
  L.sel_out = h->st.d_sel;
  L.costs_host = nullptr;
  L.sel_host = nullptr;
  L.arena_host = nullptr;
  L.arena_dev = nullptr;
  L.arena_bytes = 0;
  if (h->st.stop_on) {
    L.stop_on = 1;
    L.stop_max_steps = h->st.stop.max_steps;
    L.stop_cap = h->st.stop_cap;
    L.stop_dec_x = h->st.stop.dec_x;
    L.stop_dec_y = h->st.stop.dec_y;
    L.stop_dec_theta = h->st.stop.dec_theta;
    L.stop_tail = h->stop_tail.p;
    L.stop_steps = h->stop_steps.p;
    L.stop_hit = h->stop_hit.p;
  }
  if (h->st.path_on) {
    L.path_on = 1;
    L.path_n_seg = static_cast<int32_t>(h->st.path_segs.size());
    // Slices of 64 segments over the grid's z where the launch leaves the GPU idle (at most 65 536 poses: a control cycle's
    // 45 x 40, a few thousand MPPI rollouts) and the path has more than two slices' worth: measured at 5 x 9 samples and
    // 1024 points, one thread per pose took 82.3 us, more than the rest of the cycle (profiles/r25_path_term.txt).  SFW_PATH_SLICES=0 keeps one thread per pose.
    const int64_t poses = count * static_cast<int64_t>(L.S);
    if (h->cfg.path_slices_on && L.path_n_seg > 128 && poses <= 65536) L.path_slices = (L.path_n_seg + 63) / 64;
    L.path_seg = h->path_seg.p;
    L.path_D = h->path_D.p;
    L.path_p = h->path_p.p;
  }
}

// ---- shared-prefix plan ---------------------------------------------------
// reference sfw_planner.hpp:457-463, the recurrence K1a runs on the device (same IEEE operations)
double new_velocity_host(double vg, double vi, double a_max, double dt) {
  if ((vg - vi) >= 0) return std::fmin(vg, vi + a_max * dt);
  return std::fmax(vg, vi - a_max * dt);
}

// Classes of the samples' velocity sequences after 1..max_p steps: cls[p-1][i] is the class of
// sample value i when the first p velocities are compared, counts[p-1] the number of classes.
// Stops early once every value is its own class (nothing left to share from there on): cls/counts
// may hold fewer than max_p levels.  new_velocity is monotone in the target (and in the previous
// velocity), hence so is every v_p, and the samples that share a sequence are CONTIGUOUS when ordered
// by target — one sort up front, then a run-length pass per level.  (Were they not, the result would
// only be more classes, never a wrong merge: two samples share a class only if all their compared
// velocities are bit-equal.)  This is the GENERIC form — every sample walks the recurrence —, the
// definition the closed form below (axis_classes::build_fast) is tested against
// (tests/test_prefix_plan.py) and the fallback for the inputs that form does not take.
void velocity_classes(const std::vector<double> &targets, double v0, double a_max, double dt, int max_p,
                      std::vector<std::vector<int32_t>> &cls, std::vector<int32_t> &counts) {
  const size_t n = targets.size();
  std::vector<int32_t> order(n);
  for (size_t i = 0; i < n; ++i) order[i] = static_cast<int32_t>(i);
  std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
    return targets[static_cast<size_t>(a)] != targets[static_cast<size_t>(b)] ? targets[static_cast<size_t>(a)] < targets[static_cast<size_t>(b)]
                                                                                : a < b;
  });
  std::vector<double> t(n), v(n, v0);
  for (size_t k = 0; k < n; ++k) t[k] = targets[static_cast<size_t>(order[k])];
  std::vector<int32_t> cur(n, 0), nxt(n);
  cls.clear();
  counts.clear();
  for (int p = 0; p < max_p; ++p) {
    int32_t id = -1;
    uint64_t prev_bits = 0;
    for (size_t k = 0; k < n; ++k) {
      v[k] = new_velocity_host(t[k], v[k], a_max, dt);
      uint64_t bits;
      std::memcpy(&bits, &v[k], sizeof(bits));
      if (k == 0 || cur[k] != cur[k - 1] || bits != prev_bits) ++id;
      nxt[k] = id;
      prev_bits = bits;
    }
    cur.swap(nxt);
    cls.emplace_back(n);
    std::vector<int32_t> &out = cls.back();
    for (size_t k = 0; k < n; ++k) out[static_cast<size_t>(order[k])] = cur[k];
    counts.push_back(id + 1);
    if (static_cast<size_t>(id + 1) == n) break;
  }
}

// Per-step cost of a launch of `items` work items, in units of one step of a SIMD-filling launch's wave
// round: below one wave per issue slot of the GPU the FP64 dependency chains are exposed and a step takes
// about 0.45 of a full round whatever the item count (cfg2: 10 us against 22 us), above it time is
// proportional to the waves.
double step_cost(double items, double items_per_wave, int cus) {
  const double capacity = 4.0 * cus * 5.5;  // waves resident at once: 4 SIMDs per CU x 5-6 waves (1024 SIMDs on a whole MI355X)
  const double x = items / items_per_wave / capacity;
  return x <= 1.0 ? 0.45 + 0.55 * x : x;
}

// Classes of ONE axis of the grid (velocity_classes of the linear or of the angular targets).
//
// The planning sits on the blocking call's critical path (the GPU has nothing but the pose rollout to do until the class
// tables arrive: profiles/r05_step_timeline_cfg2.txt), and the generic form above walks n x max_p recurrence steps and
// allocates a class vector per step count — 26 us for cfg2's 128 + 128 targets, 52 us for the target configuration's.
// Closed form (build_fast): with s = a_max dt > 0 every sample that has not reached its target yet carries the SAME
// velocity — u_p = fl(u_{p-1} + s) above the start velocity, d_p = fl(d_{p-1} - s) below it — and a sample that has
// reached its target keeps it:  v_p(t) = t - v0 >= 0 ? fmin(t, u_p) : fmax(t, d_p)  (induction over new_velocity_host's
// two branches; the reached sample takes the first branch with vg - vi == 0 and fmin(t, fl(t + s)) = t).  In target
// order the classes of level p are therefore
//     [0, lo_p) all t <= d_p : ONE class | [lo_p, hi_p) reached: one class per distinct target | [hi_p, n) all t >= u_p : ONE class
// with lo_p falling and hi_p rising in p: two pointers, O(n + max_p) for all the class COUNTS (what the level choice needs),
// and the class array of a level is written only when a chosen level asks for it (level()).  Taken only when the model's
// premises hold — s > 0, u and d really move at every step (no stall at an ulp), no -0.0 among the targets (the generic form
// compares bits) —, otherwise the generic form runs.  Same classes, same numbering (in target order) as the generic form.
struct axis_classes {
  std::vector<int32_t> n;               // class counts per number of compared steps (index p - 1)
  // what they were derived from (a shared copy is only reused for exactly these inputs)
  std::vector<double> targets;
  double v0 = 0, a_max = 0, dt = 0;
  int max_p = 0;
  bool made_for(const std::vector<double> &t, double v0_, double a_, double dt_, int mp) const {
    return v0 == v0_ && a_max == a_ && dt == dt_ && max_p == mp && targets == t;
  }
  // class of every value when the first p velocities are compared (p >= 1; past the last computed level: that level, where
  // every value is its own class)
  const std::vector<int32_t> &level(int p) const {
    const size_t l = std::min<size_t>(static_cast<size_t>(p), n.size()) - 1;
    if (!fast) return c[l];
    if (c[l].empty()) write_level(l);
    return c[l];
  }
  // (a copy lent to several threads — sfw_multi_score_grid's column axis — is completed first: level() then only reads)
  void complete() const {
    if (fast)
      for (size_t l = 0; l < n.size(); ++l)
        if (c[l].empty()) write_level(l);
  }
  bool fast = false;

  void build(bool allow_fast) {
    fast = allow_fast && build_fast();
    if (!fast) {
      c.clear();
      velocity_classes(targets, v0, a_max, dt, max_p, c, n);
    }
  }

 private:
  mutable std::vector<std::vector<int32_t>> c;  // generic: every level; fast: the levels asked for so far
  std::vector<int32_t> order;                   // fast: target order -> value index
  std::vector<int32_t> run;                     // fast: run (distinct bit pattern) of every position in target order, from 0
  std::vector<int32_t> lo, hi;                  // fast: per level
  static uint64_t bits_of(double x) {
    uint64_t b;
    std::memcpy(&b, &x, sizeof(b));
    return b;
  }
  bool build_fast() {
    const size_t cnt = targets.size();
    n.clear();
    c.clear();
    lo.clear();
    hi.clear();
    if (cnt == 0 || max_p < 1) return false;
    const double s = a_max * dt;
    if (!(s > 0.0) || !std::isfinite(s) || !std::isfinite(v0)) return false;
    for (double t : targets)
      if (!std::isfinite(t) || bits_of(t) == (uint64_t(1) << 63)) return false;
    order.resize(cnt);
    bool sorted = true;
    for (size_t i = 0; i < cnt; ++i) {
      order[i] = static_cast<int32_t>(i);
      if (i && targets[i] < targets[i - 1]) sorted = false;
    }
    if (!sorted)
      std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        return targets[static_cast<size_t>(a)] != targets[static_cast<size_t>(b)] ? targets[static_cast<size_t>(a)] < targets[static_cast<size_t>(b)]
                                                                                    : a < b;
      });
    auto t_at = [&](size_t k) { return targets[static_cast<size_t>(order[k])]; };
    run.resize(cnt);
    int32_t r = 0;
    for (size_t k = 0; k < cnt; ++k) {
      if (k && bits_of(t_at(k)) != bits_of(t_at(k - 1))) ++r;
      run[k] = r;
    }
    size_t m = 0;  // first position of the side that accelerates (vg - vi >= 0 at the start velocity)
    while (m < cnt && !((t_at(m) - v0) >= 0)) ++m;
    double u = v0, d = v0;
    size_t l = m, h = m;  // lo_p / hi_p: the reached zone [l, h) grows from the start velocity outwards
    for (int p = 0; p < max_p; ++p) {
      // the recurrence's own expressions (new_velocity_host): vi + a_max * dt, vi - a_max * dt
      const double un = u + a_max * dt, dn = d - a_max * dt;
      if (!(un > u) || !(dn < d) || !std::isfinite(un) || !std::isfinite(dn)) return false;  // stalled at an ulp: generic form
      u = un;
      d = dn;
      while (h < cnt && t_at(h) < u) ++h;       // t < u_p: reached (fmin(t, u_p) = t); t >= u_p: carries u_p
      while (l > 0 && t_at(l - 1) > d) --l;     // t > d_p: reached; t <= d_p: carries d_p
      lo.push_back(static_cast<int32_t>(l));
      hi.push_back(static_cast<int32_t>(h));
      // classes: the group below (if any) + the distinct targets in [l, h) + the group above (if any).  A target equal to
      // u_p (d_p) carries the group's value: it sits in the group (h stops in front of it)
      int32_t classes = (l > 0 ? 1 : 0) + (h < cnt ? 1 : 0);
      if (h > l) classes += run[h - 1] - run[l] + 1;
      n.push_back(classes);
      if (static_cast<size_t>(classes) == cnt) break;
    }
    c.assign(n.size(), std::vector<int32_t>());
    return true;
  }
  void write_level(size_t lv) const {
    const size_t cnt = targets.size();
    const size_t l = static_cast<size_t>(lo[lv]), h = static_cast<size_t>(hi[lv]);
    std::vector<int32_t> &out = c[lv];
    out.resize(cnt);
    const int32_t below = l > 0 ? 1 : 0;
    const int32_t mid = h > l ? run[h - 1] - run[l] + 1 : 0;
    for (size_t k = 0; k < cnt; ++k) {
      int32_t id;
      if (k < l) id = 0;
      else if (k < h) id = below + (run[k] - run[l]);
      else id = below + mid;
      out[static_cast<size_t>(order[k])] = id;
    }
  }
};
// SFW_PLAN_GENERIC=1 in the environment: always the generic form (A/B and tests)
bool plan_fast_allowed() {
  static const bool on = [] {
    const char *e = std::getenv("SFW_PLAN_GENERIC");
    return !(e && e[0] == '1');
  }();
  return on;
}
axis_classes classes_of_axis(const std::vector<double> &targets, double v0, double a_max, double dt, int max_p,
                             bool allow_fast = plan_fast_allowed()) {
  axis_classes a;
  a.targets = targets;
  a.v0 = v0;
  a.a_max = a_max;
  a.dt = dt;
  a.max_p = max_p;
  a.build(allow_fast);
  return a;
}
int prefix_max_p(int S) { return std::min(S - 1, 48); }

// Everything plan_prefix derives from the staged sample vectors alone (no device involved).  The column axis may be
// borrowed (`shared_cols`): every rank of a multi-device grid has the same angular targets.
struct prefix_classes {
  axis_classes rows, own_cols;
  const axis_classes *cols = nullptr;
  int max_p = 0;
  // a level past the last computed one has every value in its own class
  int32_t n_rows_at(int p) const { return rows.n[std::min<size_t>(static_cast<size_t>(p), rows.n.size()) - 1]; }
  int32_t n_cols_at(int p) const { return cols->n[std::min<size_t>(static_cast<size_t>(p), cols->n.size()) - 1]; }
  // The WORK ITEMS of a level ending at step p are row classes(p) x column classes(p - 1): the robot records of steps
  // 0..p-1 hold positions, and the position after step i takes the heading BEFORE the step (ref :586-588) — the angular
  // velocities of steps 0..i-1 only —, so the column axis lags the row axis by one step.  p = 1: no angular velocity has
  // acted yet, one column class.
  int32_t n_item_cols_at(int p) const { return p >= 2 ? n_cols_at(p - 1) : 1; }
  const std::vector<int32_t> &item_cols(int p) const { return p >= 2 ? cols->level(p - 1) : one_col; }
  int64_t n_items_at(int p) const { return static_cast<int64_t>(n_rows_at(p)) * n_item_cols_at(p); }
  std::vector<int32_t> one_col;  // every column in class 0
};

void classes_of_grid(prefix_classes &pc, const std::vector<double> &lin, const std::vector<double> &ang, double vx0,
                     double vth0, double acc_x, double acc_theta, double dt, int S, const axis_classes *shared_cols = nullptr) {
  pc.max_p = prefix_max_p(S);
  pc.rows = classes_of_axis(lin, vx0, acc_x, dt, pc.max_p);
  if (shared_cols && shared_cols->made_for(ang, vth0, acc_theta, dt, pc.max_p)) {
    pc.cols = shared_cols;
  } else {
    pc.own_cols = classes_of_axis(ang, vth0, acc_theta, dt, pc.max_p);
    pc.cols = &pc.own_cols;
  }
  pc.one_col.assign(ang.size(), 0);
}

// The levels' end steps.  A level ending at step p costs (p - q) steps over items(p) = rows(p) x columns(p - 1) plus a
// launch and the class records (0.4 to 1.0 of a round); the suffix costs (S - p) steps over all
// samples.  Dynamic programme over the end step of the last level; empty when sharing does not pay.
std::vector<int> choose_levels(const prefix_classes &pc, int64_t T, int S, double samples_per_wave, int cus) {
  std::vector<int> steps;
  const double full = step_cost(static_cast<double>(T), samples_per_wave, cus);
  // (the column axis lags by one step: its last computed level is the items' axis one step later)
  const int last_p = std::min<int>(pc.max_p, static_cast<int>(std::max(pc.rows.n.size(), pc.cols->n.size() + 1)));
  std::vector<double> best(static_cast<size_t>(last_p) + 1, 0.0);
  std::vector<int> from(static_cast<size_t>(last_p) + 1, 0);
  double best_total = S * full;
  int best_end = 0;
  for (int p = 1; p <= last_p; ++p) {
    const double c = step_cost(static_cast<double>(pc.n_items_at(p)), samples_per_wave, cus);
    // per extra launch: dispatch + class records for an under-filled level; a level that fills the GPU
    // also pays its ramp-up and tail (measured: 0.4 / 1.0 pick the fastest plans at cfg2 / target)
    const double launch_cost = c < 1.0 ? 0.4 : 1.0;
    best[p] = 1e300;
    for (int q = 0; q < p; ++q) {
      const double v = best[q] + (p - q) * c + launch_cost;
      if (v < best[p]) { best[p] = v; from[p] = q; }
    }
    const double total = best[p] + (S - p) * full;
    if (total < best_total) { best_total = total; best_end = p; }
  }
  if (best_total > 0.97 * S * full) return steps;  // not worth the extra launches
  for (int p = best_end; p > 0; p = from[p]) steps.push_back(p);
  std::reverse(steps.begin(), steps.end());
  return steps;
}

// Row blocks of (about) equal PLANNED work for R ranks.  A block's work is its class-steps through the shared-prefix
// levels plus its samples' remaining steps, and the share of steps the tree saves differs along the row axis (rows are
// ordered by target velocity: cfg5 cut into 8 equal blocks integrates 64 %..76 % of its steps per block).  With the
// levels of the whole grid's plan every row gets a weight — for each level, (steps of the level) x (the items' column classes) if
// the row opens a new row class at that level, plus nw x (S - split) for its samples' own steps — and the cuts go where
// the running sum passes r/R of the total.  Equal row counts when nothing is shared.  Each rank still makes its own plan
// for its block; costs do not depend on the cut.
void plan_row_blocks(const std::vector<double> &lin, const std::vector<double> &ang, double vx0, double vth0, double acc_x,
                     double acc_theta, double dt, int S, int A, int R, int form, int cus, std::vector<int32_t> &row0) {
  const int64_t nv = static_cast<int64_t>(lin.size()), nw = static_cast<int64_t>(ang.size());
  row0.assign(static_cast<size_t>(R) + 1, 0);
  for (int r = 0; r <= R; ++r) row0[static_cast<size_t>(r)] = static_cast<int32_t>((static_cast<int64_t>(r) * nv) / R);
  if (R <= 1 || A < 2 || S < 2 || (nv / R) * nw < 4096) return;
  prefix_classes pc;
  classes_of_grid(pc, lin, ang, vx0, vth0, acc_x, acc_theta, dt, S);
  // the levels of the WHOLE grid's plan (its class counts are the whole grid's): the blocks' own plans differ in detail,
  // the relative weights along the row axis do not
  const std::vector<int> steps = choose_levels(pc, nv * nw, S, static_cast<double>(sfw_samples_per_wave(A, (nv / R) * nw, form, cus)), cus);
  if (steps.empty()) return;
  std::vector<double> w(static_cast<size_t>(nv), static_cast<double>(nw) * (S - steps.back()));
  int prev = 0;
  for (int p : steps) {
    const std::vector<int32_t> &rc = pc.rows.level(p);
    const double per_class = static_cast<double>(pc.n_item_cols_at(p)) * (p - prev);
    for (int64_t i = 0; i < nv; ++i)
      if (i == 0 || rc[static_cast<size_t>(i)] != rc[static_cast<size_t>(i - 1)]) w[static_cast<size_t>(i)] += per_class;
    prev = p;
  }
  double total = 0.0;
  for (double v : w) total += v;
  double run = 0.0;
  int r = 1;
  for (int64_t i = 0; i < nv && r < R; ++i) {
    run += w[static_cast<size_t>(i)];
    while (r < R && run >= total * r / R) row0[static_cast<size_t>(r++)] = static_cast<int32_t>(i + 1);
  }
  for (; r < R; ++r) row0[static_cast<size_t>(r)] = static_cast<int32_t>(nv);
}

// Decide the levels of the staged grid's shared-prefix tree and lay the class tables out per chunk of
// whole rows.
int plan_prefix(sfw_handle h, int64_t chunk, int S) {
  h->st.prefix_steps.clear();
  h->st.prefix_chunks.clear();
  h->st.cls_ints.clear();
  h->st.cls_max = 0;
  h->st.prefix_class_steps = h->st.prefix_last_classes = 0;
  const int64_t T = static_cast<int64_t>(h->st.nv) * h->st.nw;
  const bool forced = !h->cfg.prefix_env.empty();
  if (h->st.list) return SFW_OK;  // a list has no axes to share a prefix along
  if ((forced && h->cfg.prefix_env[0] == 0) || h->st.A < 2 || S < 2 || h->st.vy_samp != 0.0) return SFW_OK;
  if (!forced && T < 4096) return SFW_OK;  // the GPU is not full: extra launches cost more than they save
  const int64_t rows_per_chunk = chunk / h->st.nw;
  if (rows_per_chunk < 1) return SFW_OK;  // a single row does not fit the table budget: no sharing
  prefix_classes pc;
  classes_of_grid(pc, h->st.lin, h->st.ang, h->st.rs.vx, h->st.rs.vtheta, h->st.ga.acc_x, h->st.ga.acc_theta, h->live.params.sim_time / S, S,
                  static_cast<const axis_classes *>(h->shared_cols));
  const axis_classes &rc = pc.rows;
  const std::vector<int32_t> &nr = pc.rows.n;
  auto level = [](const axis_classes &c, int p) -> const std::vector<int32_t> & { return c.level(p); };
  auto count_at = [](const std::vector<int32_t> &n, int p) { return n[std::min<size_t>(static_cast<size_t>(p), n.size()) - 1]; };
  std::vector<int> steps;
  if (forced) {
    for (int p : h->cfg.prefix_env)
      if (p >= 1 && p <= pc.max_p) steps.push_back(p);
  } else {
    steps = choose_levels(pc, T, S, static_cast<double>(sfw_samples_per_wave(h->st.A, std::min<int64_t>(T, rows_per_chunk * h->st.nw), h->live.k2_form, h->cfg.n_cu)), h->cfg.n_cu);
  }
  if (steps.empty()) return SFW_OK;
  const size_t n_lv = steps.size();

  // ---- tables: columns (chunk-independent), then rows per chunk
  std::vector<int32_t> ints;
  ints.swap(h->st.cls_ints);  // (reuse the last stage's allocation)
  ints.clear();
  ints.reserve(static_cast<size_t>(2 * n_lv + 2) * static_cast<size_t>(h->st.nv + h->st.nw));
  auto append = [&](const std::vector<int32_t> &v) {
    const size_t o = ints.size();
    ints.insert(ints.end(), v.begin(), v.end());
    return o;
  };
  // representatives (first member) of the classes of `cls` over the index range [i0, i1); ids are
  // relabelled in order of first appearance; `local` receives the relabelled class of every index
  std::vector<int32_t> ids;  // class id -> relabelled id of the current range (ids are < the axis length)
  auto relabel = [&ids](const std::vector<int32_t> &cls, int64_t i0, int64_t i1, std::vector<int32_t> &local,
                        std::vector<int32_t> &rep) {
    ids.assign(cls.size(), -1);
    local.clear();
    rep.clear();
    local.reserve(static_cast<size_t>(i1 - i0));  // (no growth by doubling: this runs on the blocking call's critical path)
    rep.reserve(static_cast<size_t>(i1 - i0));
    for (int64_t i = i0; i < i1; ++i) {
      int32_t &id = ids[static_cast<size_t>(cls[static_cast<size_t>(i)])];
      if (id < 0) {
        id = static_cast<int32_t>(rep.size());
        rep.push_back(static_cast<int32_t>(i - i0));
      }
      local.push_back(id);
    }
  };
  struct axis_level { std::vector<int32_t> local, rep, src; };
  // levels of one axis over [i0, i1): local classes, representatives, parent classes
  // (cls null: the items' column axis, which lags the rows by one step — prefix_classes::item_cols)
  auto axis_levels = [&](const axis_classes *cls, int64_t i0, int64_t i1) {
    std::vector<axis_level> out(n_lv);
    for (size_t l = 0; l < n_lv; ++l) {
      relabel(cls ? level(*cls, steps[l]) : pc.item_cols(steps[l]), i0, i1, out[l].local, out[l].rep);
      if (l > 0) {  // classes refine: the parent of a class is the previous level's class of its representative
        out[l].src.reserve(out[l].rep.size());
        for (int32_t r : out[l].rep) out[l].src.push_back(out[l - 1].local[static_cast<size_t>(r)]);
      }
    }
    return out;
  };
  const std::vector<axis_level> cols = axis_levels(nullptr, 0, h->st.nw);
  std::vector<size_t> o_col_rep(n_lv), o_col_src(n_lv);
  for (size_t l = 0; l < n_lv; ++l) {
    o_col_rep[l] = append(cols[l].rep);
    o_col_src[l] = append(cols[l].src);
  }
  h->st.prefix_o_col_cls = append(cols[n_lv - 1].local);
  int64_t max_cls = 0;
  for (int64_t r0 = 0; r0 < h->st.nv; r0 += rows_per_chunk) {
    const int64_t r1 = std::min<int64_t>(h->st.nv, r0 + rows_per_chunk);
    const std::vector<axis_level> rows = axis_levels(&rc, r0, r1);
    chunk_plan cp;
    for (size_t l = 0; l < n_lv; ++l) {
      level_tables t;
      t.n_row = static_cast<int32_t>(rows[l].rep.size());
      t.n_col = static_cast<int32_t>(cols[l].rep.size());
      t.o_row_rep = append(rows[l].rep);
      t.o_row_src = append(rows[l].src);
      t.o_col_rep = o_col_rep[l];
      t.o_col_src = o_col_src[l];
      cp.lv.push_back(t);
      const int64_t n = static_cast<int64_t>(t.n_row) * t.n_col;
      max_cls = std::max(max_cls, n);
      h->st.prefix_class_steps += n * (steps[l] - (l ? steps[l - 1] : 0));
      if (l + 1 == n_lv) h->st.prefix_last_classes += n;
    }
    cp.o_row_cls = append(rows[n_lv - 1].local);
    h->st.prefix_chunks.push_back(cp);
  }
  // (host only: the tables reach the device with the stage's one arena copy — stage_common — or, when a launch re-plans
  // after sfw_set_params, by a copy of their own: upload_class_tables)
  h->st.cls_ints.swap(ints);
  h->st.cls_max = max_cls;
  h->st.cls_two = n_lv > 1;
  if (std::getenv("SFW_DEBUG_PLAN")) {
    std::fprintf(stderr, "[sfw] shared prefix, %d x %d samples, S=%d, %zu chunk(s):", h->st.nv, h->st.nw, S, h->st.prefix_chunks.size());
    for (size_t l = 0; l < n_lv; ++l)
      std::fprintf(stderr, " [%d,%d) %d x %d;", l ? steps[l - 1] : 0, steps[l], count_at(nr, steps[l]), pc.n_item_cols_at(steps[l]));
    std::fprintf(stderr, " [%d,%d) samples\n", steps.back(), S);
  }
  h->st.prefix_steps = steps;
  h->st.prefix_S = S;
  h->st.prefix_chunk = rows_per_chunk * h->st.nw;
  return SFW_OK;
}

// Pairs with w x diff == 0 exactly, w = v_i - v_j: relative rest (two standing people, a stopped robot next to a
// standing person) and motion exactly along the connecting line (two people on one grid-aligned line walking towards
// or away from each other).  There the model's interaction angle theta is mathematically 0 or +-pi and its angular
// term -sign(theta) exp(-d/B - (n B theta)^2) leftNormal(Ihat) is discontinuous.  The kernels take sign(theta) from
// w x diff, exactly 0 here, and their angular term is then exactly 0.  lightsfm instead forms theta as the difference of two
// atan2 — of vectors equal up to rounding when I = lambda w + dhat points along dhat (sign(theta) = -1, 0 or +1 by the
// rounding of the HOST's libm: a full-magnitude lateral force on an ordinary scene), of opposite vectors when the pair
// separates faster than 1/lambda (theta = +-pi by the sign of a zero).  Such a configuration can only come from the state
// the caller hands over (from step 1 on every agent has been pushed by a different force — the reference's own lateral
// term breaks the alignment), and that state is the same for every sample, so this term is evaluated here, once per
// stage, with the same expression sequence and the same libm the reference would run on this host (SURVEY.md Appendix
// A: computeSocialForce), and added to the agents' starting forces.  Bug-compatibility with the restated text of an
// unpinned dependency, not a CPU path: no sample is scored on the host.  out: A x (fx, fy).
void rest_forces(const sfw_params &p, const std::vector<std::pair<int32_t, int32_t>> &pairs, const double *pos, const double *vel,
                 int A, double *out) {
  for (int i = 0; i < 2 * A; ++i) out[i] = 0.0;
  for (const auto &pr : pairs) {
    const int i = pr.first, j = pr.second;
    const double dx = pos[2 * j] - pos[2 * i], dy = pos[2 * j + 1] - pos[2 * i + 1];  // diff = other - me
    const double dn = std::sqrt(dx * dx + dy * dy);
    if (!(dn > 0.0)) continue;
    const double ux = dx / dn, uy = dy / dn;                                          // diffDirection
    const double wx = vel[2 * i] - vel[2 * j], wy = vel[2 * i + 1] - vel[2 * j + 1];  // velDiff (= 0)
    const double ix = p.sfm_lambda * wx + ux, iy = p.sfm_lambda * wy + uy;            // interactionVector
    const double il = std::sqrt(ix * ix + iy * iy);
    if (!(il > 0.0)) continue;  // I = 0 (apart at exactly 1/lambda along the line): the reference divides by zero there; the kernels' term is 0
    const double ex = ix / il, ey = iy / il;                                          // interactionDirection
    double theta = std::atan2(uy, ux) - std::atan2(ey, ex);                           // angleTo, kept in (-pi, pi]
    while (theta <= -M_PI) theta += 2.0 * M_PI;
    while (theta > M_PI) theta -= 2.0 * M_PI;
    const double B = p.sfm_gamma * il;
    if (theta != 0.0) {
      const double sq = p.sfm_n * B * theta;
      const double fa = -(theta > 0.0 ? 1.0 : -1.0) * std::exp(-dn / B - sq * sq);
      out[2 * i] += p.sfm_force_factor_social * fa * -ey;                             // leftNormal = (-y, x)
      out[2 * i + 1] += p.sfm_force_factor_social * fa * ex;
    }
  }
}

// A person that can never move (desired_velocity == 0: lightsfm's speed clamp sets its velocity to 0 in every updatePosition)
// next to a robot that stands still for the whole rollout (twist 0 at hand-over, sample (0, w): it may turn, its agent
// velocity — the robot-LOCAL twist, ref :600-604 — and its position stay what they are) is at exact relative rest at EVERY
// step, not only in the handed-over state: lightsfm's sign(theta) is the rounding noise of two atan2 there (0 for most
// geometries, +-1 — a full-magnitude lateral term in Wr and Wp — for the others), the kernels' is 0.  The geometry
// of such a pair is the same at every step of every such sample — robot at (rs.x, rs.y), person where it stands — so, like
// rest_forces for the handed-over state, the host evaluates the reference's expression once per stage:
//   out[0..1] = the robot position the table holds for (the kernels compare a step's robot record with it, bit for bit)
//   out[2..3] = sum over the pinned people k of the LATERAL part of the force k exerts on the robot (joins the robot's social
//               force of the step AFTER every step whose post-step robot record is that position at velocity 0)
//   out[4+i]  = |force the robot exerts on person i| with the lateral part minus the same without it — what the kernels' Wp
//               of person i lacks at every such step; 0 for a person that can move or that carries the robot's id (ref :692).
// Returns false when no person is pinned (no table).  A robot that BRAKES to a stop during the rollout stands at a position
// the device's own pose rollout produced; the rounding noise at that position is not reproduced.
bool pinned_rest_table(const sfw_params &p, const sfw_robot_state &rs, const double *pos, const sfw_agent_const *cst, int A,
                       double *out) {
  bool any = false;
  for (int i = 1; i < A; ++i) any |= (cst[i].desired_velocity == 0.0);
  if (!any) return false;
  out[0] = rs.x;
  out[1] = rs.y;
  out[2] = out[3] = 0.0;
  for (int i = 0; i < A; ++i) out[4 + i] = 0.0;
  // force exerted on `me` by `other`, both at velocity 0 (lightsfm computeSocialForce, one term):
  // the whole term in (fx, fy), its angular part in (lx, ly)
  auto pair_at_rest = [&](double mx, double my, double ox, double oy, double &fx, double &fy, double &lx, double &ly) {
    fx = fy = lx = ly = 0.0;
    const double dx = ox - mx, dy = oy - my;
    const double dn = std::sqrt(dx * dx + dy * dy);
    if (!(dn > 0.0)) return;
    const double ux = dx / dn, uy = dy / dn;                  // diffDirection
    const double ix = p.sfm_lambda * 0.0 + ux, iy = p.sfm_lambda * 0.0 + uy;  // interactionVector, velDiff = 0
    const double il = std::sqrt(ix * ix + iy * iy);
    if (!(il > 0.0)) return;
    const double ex = ix / il, ey = iy / il;                  // interactionDirection
    double theta = std::atan2(uy, ux) - std::atan2(ey, ex);   // angleTo, kept in (-pi, pi]
    while (theta <= -M_PI) theta += 2.0 * M_PI;
    while (theta > M_PI) theta -= 2.0 * M_PI;
    const double B = p.sfm_gamma * il;
    const double sv = p.sfm_n_prime * B * theta, sa = p.sfm_n * B * theta;
    const double fv = -std::exp(-dn / B - sv * sv);
    const double sg = theta > 0.0 ? 1.0 : theta < 0.0 ? -1.0 : 0.0;
    const double fa = -sg * std::exp(-dn / B - sa * sa);
    lx = p.sfm_force_factor_social * (fa * -ey);              // leftNormal = (-y, x)
    ly = p.sfm_force_factor_social * (fa * ex);
    fx = p.sfm_force_factor_social * (fv * ex + fa * -ey);
    fy = p.sfm_force_factor_social * (fv * ey + fa * ex);
  };
  for (int i = 1; i < A; ++i) {
    if (cst[i].desired_velocity != 0.0) continue;
    double fx, fy, lx, ly;
    pair_at_rest(rs.x, rs.y, pos[2 * i], pos[2 * i + 1], fx, fy, lx, ly);  // on the robot, by person i
    out[2] += lx;
    out[3] += ly;
    pair_at_rest(pos[2 * i], pos[2 * i + 1], rs.x, rs.y, fx, fy, lx, ly);  // on person i, by the robot
    if (cst[i].id != cst[0].id) out[4 + i] = std::sqrt(fx * fx + fy * fy) - std::sqrt((fx - lx) * (fx - lx) + (fy - ly) * (fy - ly));
  }
  return true;
}

// Everything of a stage that depends on sfw_params: the K1->K2 tables ([S][chunk] records, chunk bounded
// by the table budget) and the shared-prefix plan (classes of the velocity sequences under dt = sim_time/S).
// The one configuration whose reference result the kernels do not reproduce (sfw_plan_info.rest_noise_unreproduced, DESIGN.md
// §10): a person that can never move next to a robot that moves now and brakes to a stop inside some sample's rollout.
// Decided from what the stage uploaded, with the device's own velocity recurrence (plain IEEE operations).
bool rest_noise_unreproduced(sfw_handle h) {
  // A perturbed stage: the host never sees the knots, so the answer is conservative — some sample may be commanded to rest
  // wherever the clamp box admits a zero translation command.
  if (h->st.valid && h->st.perturbed) return h->st.person_pinned && h->st.A >= 2 && h->st.zero_admitted;
  if (h->st.valid && h->st.nk > 1) {
    // Sequences: a sample can come to rest behind a knot, or start to move at one.  The host walks every sample's own
    // recurrence over the knots — only when a person is pinned — and flags a translation velocity that REACHES (0, 0) after a
    // step i < S - 1 having been non-zero at hand-over or after an earlier step.  A robot that stands from hand-over and starts
    // to move at a later knot is at rest only at the handed-over pose, which the pinned-rest table covers step by step.
    if (h->st.A < 2 || !h->st.person_pinned) return false;
    const int S = num_steps_of(h->live.params);
    const double dt = h->live.params.sim_time / S;
    const size_t n = static_cast<size_t>(h->st.nv);
    for (size_t t = 0; t < n; ++t) {
      double vx = h->st.rs.vx, vy = h->st.rs.vy;
      bool moved = vx != 0.0 || vy != 0.0;
      int k = 0;
      for (int i = 0; i + 1 < S; ++i) {
        if (k + 1 < h->st.nk && h->st.knot_step[static_cast<size_t>(k) + 1] == i) ++k;
        const size_t at = static_cast<size_t>(k) * n + t;
        vx = new_velocity_host(h->st.lin[at], vx, h->st.ga.acc_x, dt);
        vy = new_velocity_host(h->st.vy.empty() ? 0.0 : h->st.vy[at], vy, h->st.ga.acc_y, dt);
        if (vx == 0.0 && vy == 0.0) {
          if (moved) return true;
        } else {
          moved = true;
        }
      }
    }
    return false;
  }
  if (!h->st.valid || h->st.A < 2 || (h->st.rs.vx == 0.0 && h->st.rs.vy == 0.0)) return false;  // (standing from the start: reproduced)
  if (!h->st.person_pinned || h->st.vy_samp != 0.0) return false;
  bool zero_row = false;
  if (h->st.list) {  // a sample that decelerates both translations to 0: vx == 0 && vy == 0
    for (size_t t = 0; t < h->st.lin.size(); ++t) zero_row |= (h->st.lin[t] == 0.0 && (h->st.vy.empty() || h->st.vy[t] == 0.0));
  } else {
    for (double v : h->st.lin) zero_row |= (v == 0.0);
  }
  if (!zero_row) return false;
  const int S = num_steps_of(h->live.params);
  const double dt = h->live.params.sim_time / S;
  double vx = h->st.rs.vx, vy = h->st.rs.vy;
  for (int i = 0; i + 1 < S; ++i) {  // at rest AFTER step i < S - 1: at least one step is integrated from the rest pose
    vx = new_velocity_host(0.0, vx, h->st.ga.acc_x, dt);
    vy = new_velocity_host(0.0, vy, h->st.ga.acc_y, dt);
    if (vx == 0.0 && vy == 0.0) return true;
  }
  return false;
}

// Rows of the stop check's tail table: a bound on the tail length of every sample of the staged grid.  A velocity never
// leaves the interval between its start and its targets, so an axis that starts the tail at |v| <= vmax is at 0 after at most
// ceil(vmax / (dec dt)) + 1 steps (the + 1: the quotient's rounding, and the recurrence's own); the tail ends when vx and vy
// both are.  vmax: over the robot's velocity and every knot's target — the clamp box for knots drawn on the device.  An axis
// that cannot brake (dec dt == 0) or a box without a finite side: max_steps.  (The kernel checks a longer tail all the same.)
int stop_axis_bound(double vmax, double dec, double dt, int max_steps) {
  if (vmax == 0.0) return 0;
  const double step = dec * dt;
  if (!(step > 0.0) || !std::isfinite(vmax)) return max_steps;
  const double q = std::ceil(vmax / step) + 1.0;
  return q < max_steps ? static_cast<int>(q) : max_steps;
}
int stop_tail_bound(sfw_handle h, int S) {
  const auto &st = h->st;
  const double dt = h->live.params.sim_time / S;
  double mx = std::fabs(st.rs.vx), my = std::fabs(st.rs.vy);
  if (st.perturbed) {
    mx = std::fmax(mx, std::fmax(std::fabs(st.pert.lo[0]), std::fabs(st.pert.hi[0])));
    my = std::fmax(my, std::fmax(std::fabs(st.pert.lo[1]), std::fabs(st.pert.hi[1])));  // (also of a stage without a vy row: only rows)
    if (std::isnan(mx) || std::isnan(my)) return st.stop.max_steps;
  } else {
    for (double v : st.lin) mx = std::fmax(mx, std::fabs(v));
    for (double v : st.vy) my = std::fmax(my, std::fabs(v));
    my = std::fmax(my, std::fabs(st.vy_samp));
  }
  return std::max(stop_axis_bound(mx, st.stop.dec_x, dt, st.stop.max_steps), stop_axis_bound(my, st.stop.dec_y, dt, st.stop.max_steps));
}

// The segment records of a path (sfw_hip.h "the path term"): n - 1 segments of n points, one zero-length segment of one point.
// The pragma keeps the host compiler from contracting ex*ex + ey*ey into a fused multiply-add: every operation is rounded
// once, as path.py and the header state it.
void path_segments(const std::vector<double> &xy, std::vector<sfw_path_seg> &out) {
#pragma clang fp contract(off)
  const size_t n = xy.size() / 2;
  out.clear();
  for (size_t i = 0; i + 1 < n || (n == 1 && i == 0); ++i) {
    const size_t j = n == 1 ? 0 : i + 1;
    const double ax = xy[2 * i], ay = xy[2 * i + 1];
    const double ex = xy[2 * j] - ax, ey = xy[2 * j + 1] - ay;
    const double len2 = ex * ex + ey * ey;
    out.push_back(sfw_path_seg{ax, ay, ex, ey, len2 > 0.0 ? 1.0 / len2 : 0.0});
  }
}

// Host half: chunk size under the table budget and the shared-prefix plan (class tables in h->st.cls_ints).  No device call.
int64_t plan_tables_host(sfw_handle h, int *err) {
  const int64_t T = static_cast<int64_t>(h->st.nv) * h->st.nw;
  const int S = num_steps_of(h->live.params);
  h->st.early_poses = false;
  h->st.stop_cap = h->st.stop_on ? stop_tail_bound(h, S) : 0;
  if (h->cfg.stop_rows_max >= 0 && h->st.stop_cap > h->cfg.stop_rows_max) h->st.stop_cap = h->cfg.stop_rows_max;
  int64_t chunk = static_cast<int64_t>(
      h->cfg.table_budget_bytes / ((kTableBytesPerSampleStep + (h->st.path_on ? sizeof(double) : 0)) * S +
                                   sizeof(sfw_pose_frame) * static_cast<size_t>(h->st.stop_cap)));
  if (chunk < 1024) chunk = 1024;
  if (chunk > kRowLimit) chunk = kRowLimit;
  if (chunk > T) chunk = T;
  *err = plan_prefix(h, chunk, S);
  h->st.plan_epoch = h->live.params_epoch;
  return chunk;
}
// The arena a stage left in pinned memory only (st.arena_pending) is fetched by the blocks of the kernel that carries L ...
void arena_by_kernel(sfw_handle h, sfw_launch &L) {
  if (!h->st.arena_pending) return;
  L.arena_host = h->pin_arena.p + h->st.arena_from;
  L.arena_dev = h->arena.p + h->st.arena_from;
  L.arena_bytes = static_cast<uint32_t>(h->st.arena_bytes);
}
// ... and once that kernel is enqueued, the pinned copy is guarded like one a copy reads
hipError_t arena_fetched(sfw_handle h) {
  if (!h->st.arena_pending) return hipSuccess;
  h->st.arena_pending = false;
  return h->pin_arena.mark(h->stream);
}

// Device half: the K1->K2 tables and the class-record buffers; with may_start_poses the pose rollout of a single-chunk grid
// is enqueued here, by the STAGE (the robot's poses depend on the sample vectors alone).
int plan_tables_device(sfw_handle h, int64_t chunk, bool may_start_poses) {
  const int64_t T = static_cast<int64_t>(h->st.nv) * h->st.nw;
  const int S = num_steps_of(h->live.params);
  SFW_HIP(h, h->ptab.reserve(static_cast<size_t>(table_row_units(chunk, h->st.nw)) * S));
  SFW_HIP(h, h->cs_tab.reserve((h->st.list ? static_cast<size_t>(chunk) : static_cast<size_t>(h->st.nw)) * S));
  SFW_HIP(h, h->fcode.reserve(static_cast<size_t>(chunk) * S));
  if (h->st.stop_on) {
    SFW_HIP(h, h->stop_steps.reserve(static_cast<size_t>(T)));
    SFW_HIP(h, h->stop_hit.reserve(static_cast<size_t>(T)));
    SFW_HIP(h, h->stop_tail.reserve(static_cast<size_t>(chunk) * static_cast<size_t>(h->st.stop_cap)));
  }
  if (h->st.path_on) {
    SFW_HIP(h, h->path_p.reserve(static_cast<size_t>(T)));
    SFW_HIP(h, h->path_D.reserve(static_cast<size_t>(chunk) * S));
  }
  h->st.table_chunk = chunk;
  if (!h->st.prefix_steps.empty())
    for (size_t b = 0; b < (h->st.cls_two ? 2u : 1u); ++b) {
      SFW_HIP(h, h->cls_dead[b].reserve(static_cast<size_t>(h->st.cls_max)));
      SFW_HIP(h, h->cls_state[b].reserve(static_cast<size_t>(h->st.cls_max) * h->st.A));
    }
  // (the fused small-grid K1 is one launch with the costmap part, and may capture points)
  if (may_start_poses && chunk >= T && !sfw_rollout_is_fused(T, S)) {
    sfw_launch L;
    fill_launch(h, L, 0, T, T);
    h->st.clock_cleared = false;
    if (h->live.timing) {  // the clock probe of a timed launch is cleared by the pose rollout itself (clear_clock_probe)
      SFW_HIP(h, h->clock.reserve(4));
      L.clock_probe = h->clock.p;
      h->st.clock_cleared = true;
    }
    if (h->live.timing) SFW_HIP(h, hipEventRecord(h->ev[0], h->stream));
    h->st.early_poses_timed = h->live.timing;
    h->st.early_poses_terms = h->live.capture_terms;
    if (h->live.capture_terms) {
      SFW_HIP(h, h->terms.reserve(static_cast<size_t>(SFW_N_TERMS) * static_cast<size_t>(T)));
      L.terms = h->terms.p;
      L.terms_T = T;
    }
    arena_by_kernel(h, L);
    if (h->st.arena_pending) {  // no copy was enqueued: this kernel reads its sample vectors at their host addresses
      L.linvels = reinterpret_cast<const double *>(h->pin_arena.p + (reinterpret_cast<const char *>(h->st.d_linvels) - h->arena.p));
      L.angvels = reinterpret_cast<const double *>(h->pin_arena.p + (reinterpret_cast<const char *>(h->st.d_angvels) - h->arena.p));
      if (h->st.d_vy) L.vy_samps = reinterpret_cast<const double *>(h->pin_arena.p + (reinterpret_cast<const char *>(h->st.d_vy) - h->arena.p));
      if (h->st.d_knot_step)
        L.knot_step = reinterpret_cast<const int32_t *>(h->pin_arena.p + (reinterpret_cast<const char *>(h->st.d_knot_step) - h->arena.p));
    }
    SFW_HIP(h, sfw_launch_rollout_poses(L, h->stream));
    SFW_HIP(h, arena_fetched(h));
    h->st.early_poses = true;
  }
  return SFW_OK;
}
// The class tables by a copy of their own (a launch that re-plans after sfw_set_params: the stage's arena is on the device already)
int upload_class_tables(sfw_handle h) {
  h->st.d_cls_tab = nullptr;
  if (h->st.cls_ints.empty()) return SFW_OK;
  const size_t bytes = sizeof(int32_t) * h->st.cls_ints.size();
  SFW_HIP(h, h->d_cls.reserve(h->st.cls_ints.size()));
  SFW_HIP(h, h->pin_cls.reserve(bytes));
  std::memcpy(h->pin_cls.p, h->st.cls_ints.data(), bytes);
  SFW_HIP(h, hipMemcpyAsync(h->d_cls.p, h->pin_cls.p, bytes, hipMemcpyHostToDevice, h->stream));
  SFW_HIP(h, h->pin_cls.mark(h->stream));
  h->st.d_cls_tab = h->d_cls.p;
  return SFW_OK;
}
int flush_arena(sfw_handle h);

// Everything of a stage that depends on sfw_params, redone by a launch when sfw_set_params came in between (the reference
// re-reads its parameters every cycle, :125): a plan made for another dt would merge samples whose robot trajectories now
// differ.  Also drops the poses the stage started: they were rolled out under the old parameters.
int replan_at_launch(sfw_handle h) {
  if (int e = flush_arena(h)) return e;  // (the device copy of the rest terms is patched below)
  int err = SFW_OK;
  const int64_t chunk = plan_tables_host(h, &err);
  if (err) return err;
  if (int e = plan_tables_device(h, chunk, false)) return e;
  if (int e = upload_class_tables(h)) return e;
  if (h->st.d_agent_rest && !h->st.rest_pairs.empty()) {  // the relative-rest terms depend on the sfm parameters too
    const size_t bytes = sizeof(double) * 2 * static_cast<size_t>(h->st.A);
    SFW_HIP(h, h->pin_cls.wait());
    SFW_HIP(h, h->pin_out.reserve(bytes));
    rest_forces(h->live.params, h->st.rest_pairs, h->st.rest_pv.data(), h->st.rest_pv.data() + 2 * h->st.A, h->st.A,
                reinterpret_cast<double *>(h->pin_out.p));
    SFW_HIP(h, hipMemcpyAsync(const_cast<double *>(h->st.d_agent_rest), h->pin_out.p, bytes, hipMemcpyHostToDevice, h->stream));
    SFW_HIP(h, hipStreamSynchronize(h->stream));  // pin_out is the fetch buffer too: rare path, keep it simple
  }
  if (h->st.d_pin_rest && h->st.pin_doubles) {  // ... and so does the pinned-rest table
    const size_t bytes = sizeof(double) * h->st.pin_doubles;
    SFW_HIP(h, h->pin_cls.wait());
    SFW_HIP(h, h->pin_out.reserve(bytes));
    pinned_rest_table(h->live.params, h->st.rs, h->st.pin_pos.data(), h->st.pin_cst.data(), h->st.A, reinterpret_cast<double *>(h->pin_out.p));
    SFW_HIP(h, hipMemcpyAsync(const_cast<double *>(h->st.d_pin_rest), h->pin_out.p, bytes, hipMemcpyHostToDevice, h->stream));
    SFW_HIP(h, hipStreamSynchronize(h->stream));
  }
  return SFW_OK;
}

// The agent / laser-point set must fit one wave's LDS allocation (160 KiB per CU).
int check_lds(sfw_handle h, int A, int O, int NG, int n_grp_mem, int64_t items) {
  const size_t lds = sfw_social_lds_bytes(A, O, NG, n_grp_mem, items, h->live.k2_form, h->cfg.n_cu);
  if (A > 0 && lds > 160 * 1024)
    return fail(h, SFW_ERR_UNSUPPORTED, "agent/obstacle set does not fit the 160 KiB LDS of one CU");
  return SFW_OK;
}

constexpr size_t kMapMergeMax = size_t(64) << 10;  // costmaps up to this many cells ride in the stage's arena copy

// SFW_DEBUG_STAGE=1 in the environment: every stage / launch prints where its host time went (stderr; tuning aid)
struct host_phases {
  bool on;
  std::chrono::steady_clock::time_point t;
  std::string out;
  explicit host_phases(const char *what) {
    static const bool enabled = std::getenv("SFW_DEBUG_STAGE") != nullptr;
    on = enabled;
    if (on) {
      out = what;
      t = std::chrono::steady_clock::now();
    }
  }
  void mark(const char *name) {
    if (!on) return;
    const auto n = std::chrono::steady_clock::now();
    char b[64];
    std::snprintf(b, sizeof(b), " %s %.1f", name, std::chrono::duration<double, std::micro>(n - t).count());
    out += b;
    t = n;
  }
  ~host_phases() {
    if (on) std::fprintf(stderr, "[sfw] %s us\n", out.c_str());
  }
};

// What a perturbed stage draws its knots from (sfw_sequences_perturb_stage, checked there): stage_common reserves the knot
// regions of the arena and enqueues sfw_perturb_kernel to fill them instead of copying lin / ang / vy_list (all null then)
struct perturb_source {
  sfw_perturb_dev args;
  bool vy, keep_normals, zero_admitted;
};

// What a stage is asked to put on the device: one of the four kinds of stage_common, made by the functions below
struct stage_request {
  enum kind_t { GRID, LIST, SEQUENCES, PERTURBED } kind;
  const double *lin, *vy_list, *ang;  // null when the device draws them (PERTURBED); vy_list nullable: all 0.0
  int32_t nv, nw, nk;                 // nk rows of nv values (lin, vy_list) and of nw (a grid) or nv (a list) values (ang), knot-major
  const int32_t *knot_step;           // the nk steps at which a knot takes over (checked by the caller: sequences_refusal)
  const perturb_source *dev;
  double vy_samp;
  int skip_zero;
  int64_t index_base;
  const char *name() const {  // in messages
    return kind == PERTURBED ? "sequences_perturb_stage" : kind == SEQUENCES ? "sequences_stage" : kind == LIST ? "samples_stage" : "grid_stage";
  }
  bool is_list() const { return kind != GRID; }
  bool drawn() const { return kind == PERTURBED; }  // the device draws the sample vectors: lin == ang == null
  size_t kn() const { return static_cast<size_t>(nk); }
  size_t n_ang() const { return static_cast<size_t>(is_list() ? nv : nw); }
};
// sfw_grid_stage: nv linear x nw angular targets, the (0, 0) sample skipped
stage_request grid_request(const double *lin, int32_t nv, const double *ang, int32_t nw, int64_t index_base) {
  return {stage_request::GRID, lin, nullptr, ang, nv, nw, 1, nullptr, nullptr, 0.0, 1, index_base};
}
// sfw_score_one / sfw_score_one_crowd: a grid of 1 x 1 with its vy, never skipped
stage_request one_request(const double *vx, double vy, const double *vtheta) {
  return {stage_request::GRID, vx, nullptr, vtheta, 1, 1, 1, nullptr, nullptr, vy, 0, 0};
}
// sfw_samples_stage: a grid of n rows by one column to everything that counts samples; never the (0, 0) skip
stage_request list_request(const double *vx, const double *vy, const double *vtheta, int32_t n, int64_t index_base) {
  return {stage_request::LIST, vx, vy, vtheta, n, 1, 1, nullptr, nullptr, 0.0, 0, index_base};
}
// sfw_sequences_stage: that list with K rows of n values behind its vectors
stage_request sequences_request(const double *vx, const double *vy, const double *vtheta, int32_t n, int32_t K,
                                const int32_t *knot_step, int64_t index_base) {
  return {stage_request::SEQUENCES, vx, vy, vtheta, n, 1, K, knot_step, nullptr, 0.0, 0, index_base};
}
// sfw_sequences_perturb_stage: sequences whose rows the device draws from dev (null: a request to read the argument rules by)
stage_request perturbed_request(const perturb_source *dev, int32_t n, int32_t K, const int32_t *knot_step, int64_t index_base) {
  return {stage_request::PERTURBED, nullptr, nullptr, nullptr, n, 1, K, knot_step, dev, 0.0, 0, index_base};
}

// stage_common's argument rules as texts of their own (null: accepted), in two parts because the costmap's state check stands
// between them: an ensemble's score calls read the same ones before ANY member is staged.
const char *stage_null_refusal(const sfw_robot_state *rs, const sfw_goal_args *args, const stage_request &q) {
  if (!rs || (!q.drawn() && (!q.lin || !q.ang)) || !args || q.nv <= 0 || q.nw <= 0) return "null pointer or non-positive sample count";
  return nullptr;
}
// A NaN would come back as a NaN cost (the header promises sentinels, never NaN) and, in a sample vector, break the
// ordering the shared-prefix planner sorts by: O(nv + nw) checks
const char *stage_finite_refusal(const sfw_robot_state *rs, const sfw_goal_args *args, const stage_request &q) {
  if (!all_finite(&rs->x, 6) || !all_finite(&args->acc_x, 5) || !std::isfinite(q.vy_samp))
    return "non-finite robot state, goal argument or sample velocity";
  const size_t rows = q.kn() * static_cast<size_t>(q.nv);
  if (!q.drawn() && (!all_finite(q.lin, rows) || !all_finite(q.ang, q.kn() * q.n_ang()) || (q.vy_list && !all_finite(q.vy_list, rows))))
    return "non-finite sample velocity";
  return nullptr;
}

// The half-width r_c (cells) of the clearance window for a footprint at a resolution, or -1 when it exceeds
// kClearMaxHalfWidth: r_c = ceil(R / res) + 1 with R the largest vertex distance.  Claim: for a pose whose centre is on the
// map in cell (cx, cy), every vertex that sfw_kernels.hip footprint_cost_at converts lands in a cell within r_c of (cx, cy)
// on each axis — and, when the window [cx - r_c, cx + r_c] x [cy - r_c, cy + r_c] is on the map, on the map.
//   * A vertex's world x is x + d with d = fl(fl(qx c) - fl(qy s)), |d| <= hypot(qx, qy) hypot(c, s) (1 + 2^-51) by Cauchy-
//     Schwarz and two roundings, and hypot(c, s) <= 1 + 2^-50 for a sincos good to a few ulp: |d| <= R (1 + 2^-49).
//   * In real numbers the vertex's quotient differs from the centre's a = (x - origin) / res by d / res, and
//     floor(a + t) - floor(a) lies in [-ceil(|t|), ceil(|t|)]: at most ceil(R / res) cells.
//   * The roundings on the way (x + d, the subtraction of the origin, the division — or cell_index's product, which its 1e-9
//     guard replaces by the division whenever the two could truncate differently — and the factor above) move a quotient by
//     a few 2^-52 of its size, under 1e-8 cells for the 2^21 cells an axis may have (SFW_MAX_MAP_AXIS_CELLS): they can carry
//     a quotient across ONE more cell edge, never two.  The host's own fl(R / res) may round down onto an integer that the
//     exact quotient exceeds by the like amount.  The "+ 1" pays for all of these together (their sum is far below one cell).
//   * With the window on the map, cx - r_c >= 0, so the vertex's exact quotient is at least cx - ceil(R / res) - 1e-8 > 0: it
//     is not below the origin, and its cell is at most cx + r_c < size.  The same on y.
// A walk between two vertex cells stays inside their bounding box (line_max: the minor axis advances `add` times over `den`
// major steps), hence inside the window.  tests/test_footprint_clearance.py measures the largest offset the reference produces
// against this bound, with centres on cell edges and the farthest vertex pointing along an axis.
int clearance_half_width(const std::vector<double> &footprint, double resolution) {
  double R = 0.0;
  for (size_t i = 0; i + 1 < footprint.size(); i += 2) R = std::fmax(R, std::hypot(footprint[i], footprint[i + 1]));
  const double q = std::ceil(R / resolution) + 1.0;
  return q <= kClearMaxHalfWidth ? static_cast<int>(q) : -1;  // (written so that a NaN or an infinite quotient gives -1)
}

// The stage's last step before it commits: does K1b of this grid read a clearance map?  Yes when `clear_map` already describes
// the staged costmap and window, or when the grid has enough poses to pay for building it — then the two passes are enqueued
// on the handle's stream, behind the stage's copy of the cells (or the pose rollout that fetches them) and in front of every
// launch.  A build that cannot be enqueued leaves the stage without a map (every pose walks), never with a stale one.
void stage_clearance(sfw_handle h, int64_t T) {
  h->st.clear_on = false;
  h->st.clear_r = -1;
  if (!h->live.fp_clear) return;
  const map_geometry &m = h->st.map;
  const int r = clearance_half_width(h->world.footprint, m.resolution);
  h->st.clear_r = r;
  if (r < 0) return;
  auto &c = h->clr;
  if (c.valid && c.cells_gen == h->world.cells_gen && c.size_x == m.size_x && c.size_y == m.size_y && c.r == r) {
    h->st.clear_on = true;
    return;
  }
  // (an arena still pending here — a small grid's, fetched by its launch — never carries cells: the device's copy of them is an
  // earlier stage's, or the large map's own copy enqueued above)
  if (T * num_steps_of(h->live.params) < h->cfg.clear_min_poses) return;
  c.valid = false;
  const size_t n = static_cast<size_t>(m.size_x) * m.size_y;
  hipError_t e = h->clear_map.reserve(n);
  if (e == hipSuccess) e = h->clear_tmp.reserve(n);
  if (e == hipSuccess) e = sfw_launch_clearance(h->st.d_cells, m.size_x, m.size_y, r, h->clear_tmp.p, h->clear_map.p, h->stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  c = {true, h->world.cells_gen, m.size_x, m.size_y, r};
  h->st.clear_on = true;
}

int stage_common(sfw_handle h, const sfw_robot_state *rs, const sfw_goal_args *args, const stage_request &q) {
  if (!h) return SFW_ERR_INVALID_ARG;
  const std::string what = q.name();
  const auto [kind, lin, vy_list, ang, nv, nw, nk, knot_step, dev, vy_samp, skip_zero, index_base] = q;
  const size_t kn = q.kn(), n_ang = q.n_ang();
  const bool has_vy = dev ? dev->vy : vy_list != nullptr;
  if (const char *why = stage_null_refusal(rs, args, q)) return fail(h, SFW_ERR_INVALID_ARG, what + ": " + why);
  if (!h->world.have_costmap) return fail(h, SFW_ERR_STATE, what + ": no costmap set (sfw_set_costmap)");
  if (const char *why = stage_finite_refusal(rs, args, q)) return fail(h, SFW_ERR_INVALID_ARG, what + ": " + why);
  drop_stage(h);  // (valid again at the end of this function, and only there)
  host_phases ph("stage:");
  SFW_HIP(h, hipSetDevice(h->device));
  const agent_set &ag = h->world.agents;
  const map_geometry &map = h->world.map_new;
  // a large costmap that has changed goes out first, by a copy of its own that runs while the host plans and packs
  const size_t n_cells = static_cast<size_t>(map.size_x) * map.size_y;
  const bool merge = n_cells <= kMapMergeMax;
  if (h->world.cells_dirty && !merge) {
    SFW_HIP(h, h->cells.reserve(n_cells));
    SFW_HIP(h, hipMemcpyAsync(h->cells.p, h->pin_map.p, n_cells, hipMemcpyHostToDevice, h->stream));
    SFW_HIP(h, h->pin_map.mark(h->stream));
    h->world.cells_dirty = false;
  }
  ph.mark("check+setdev");
  h->st.perturbed = dev != nullptr;
  h->st.zero_admitted = dev && dev->zero_admitted;
  if (dev) h->st.pert = dev->args;
  h->st.normals_kept = false;  // (until the kernel that writes them is enqueued)
  if (dev) {  // the knots exist on the device only
    h->st.lin.clear();
    h->st.ang.clear();
  } else {
    h->st.lin.assign(lin, lin + kn * nv);
    h->st.ang.assign(ang, ang + kn * n_ang);
  }
  h->st.list = q.is_list();
  if (vy_list) h->st.vy.assign(vy_list, vy_list + kn * nv);
  else h->st.vy.clear();
  h->st.nk = static_cast<int>(kn);
  if (knot_step) h->st.knot_step.assign(knot_step, knot_step + kn);
  else h->st.knot_step.clear();
  h->st.K = h->world.K;
  h->st.clear_on = false;  // (until stage_clearance, at the end, says otherwise)
  h->st.stop_on = h->live.stop_on;
  h->st.stop = h->live.stop;
  h->st.path_on = h->live.path_on;
  h->st.path_weight = h->live.path_weight;
  if (h->st.path_on) {
    path_segments(h->live.path_xy, h->st.path_segs);
    // Unchanged records stay where they are.  Changed ones go through a pinned buffer of their own (pin_path: reserve waits
    // for the last upload, mark guards this one), like the arena; the copy is on the stream, behind the launches of an earlier
    // stage that read the old records
    const size_t seg_bytes = sizeof(sfw_path_seg) * h->st.path_segs.size();
    if (!h->path_seg.p || h->path_seg_sent.size() != h->st.path_segs.size() ||
        std::memcmp(h->path_seg_sent.data(), h->st.path_segs.data(), seg_bytes) != 0) {
      h->path_seg_sent.clear();
      SFW_HIP(h, h->pin_path.reserve(seg_bytes));
      std::memcpy(h->pin_path.p, h->st.path_segs.data(), seg_bytes);
      SFW_HIP(h, h->path_seg.reserve(h->st.path_segs.size()));
      SFW_HIP(h, hipMemcpyAsync(h->path_seg.p, h->pin_path.p, seg_bytes, hipMemcpyHostToDevice, h->stream));
      SFW_HIP(h, h->pin_path.mark(h->stream));
      h->path_seg_sent = h->st.path_segs;
    }
  } else {
    h->st.path_segs.clear();
  }
  h->st.A = ag.A;
  h->st.O = ag.O;
  h->st.NG = ag.NG;
  h->st.n_grp_mem = ag.n_grp_mem;
  h->st.person_pinned = ag.person_pinned;
  h->st.nv = nv;
  h->st.nw = nw;
  h->st.rs = *rs;
  h->st.ga = *args;
  h->st.vy_samp = vy_samp;
  h->st.skip_zero = skip_zero;
  h->st.index_base = index_base;
  h->st.map = map;
  // The shared-prefix plan FIRST, on the host (a few microseconds since round 6: axis_classes): its class tables ride in the
  // stage's one arena copy and the levels can be enqueued right behind the pose rollout.  (Rounds 1-5 planned behind the
  // arena copy and the pose rollout, 25-50 us, and sent the tables in a second copy the first level then waited for.)
  int plan_err = SFW_OK;
  const int64_t chunk = plan_tables_host(h, &plan_err);
  if (plan_err) return plan_err;
  ph.mark("plan");
  // a small costmap (<= 64 KB: a control cycle's local costmap of 200 x 200 cells) is the head of the arena and sent with
  // it when it has changed; a larger one has gone out by a copy of its own (above)
  auto up16 = [](size_t b) { return (b + 15) & ~size_t(15); };
  const size_t cells_head = merge ? up16(n_cells) : 0;
  {  // one arena, one copy: footprint | agents blob | linvels | angvels | [a list's vy] | [knot steps] | relative-rest terms | pinned-rest table | class tables
    const bool rest = !ag.rest_pairs.empty();
    const size_t o_fp = cells_head, o_ag = o_fp + up16(sizeof(double) * (h->world.footprint.empty() ? 2 : h->world.footprint.size())),
                 o_lin = o_ag + up16(ag.blob.size()), o_ang = o_lin + up16(sizeof(double) * kn * nv),
                 o_vy = o_ang + up16(sizeof(double) * kn * n_ang),
                 o_knot = o_vy + (has_vy ? up16(sizeof(double) * kn * nv) : 0),
                 o_rest = o_knot + (knot_step ? up16(sizeof(int32_t) * kn) : 0),
                 o_pin = o_rest + (rest ? up16(sizeof(double) * 2 * static_cast<size_t>(ag.A)) : 0),
                 pin_doubles = 4 + static_cast<size_t>(ag.A > 0 ? ag.A : 0),
                 // (room for the pinned-rest table whenever the robot stands still at hand-over: whether one is needed is known
                 // once the agents' constants have been looked at, below)
                 o_cls = o_pin + ((h->cfg.pin_rest_on && rs->vx == 0.0 && rs->vy == 0.0 && ag.A > 1) ? up16(sizeof(double) * pin_doubles) : 0),
                 total = o_cls + up16(sizeof(int32_t) * h->st.cls_ints.size());
    SFW_HIP(h, h->pin_arena.reserve(total));
    // (an `arena` that moves, or that this stage does not keep the cells at the head of, loses its copy of them)
    if (!merge || total > h->arena.cap) h->st.cells_in_arena = false;
    const bool send_cells = merge && (h->world.cells_dirty || !h->st.cells_in_arena || h->st.arena_cells_bytes != cells_head);
    SFW_HIP(h, h->arena.reserve(total));
    char *pb = h->pin_arena.p;
    if (send_cells) std::memcpy(pb, h->pin_map.p, n_cells);
    if (!h->world.footprint.empty()) std::memcpy(pb + o_fp, h->world.footprint.data(), sizeof(double) * h->world.footprint.size());
    if (!ag.blob.empty()) std::memcpy(pb + o_ag, ag.blob.data(), ag.blob.size());
    if (!dev) {
      std::memcpy(pb + o_lin, lin, sizeof(double) * kn * nv);
      std::memcpy(pb + o_ang, ang, sizeof(double) * kn * n_ang);
      if (vy_list) std::memcpy(pb + o_vy, vy_list, sizeof(double) * kn * nv);
    }
    if (knot_step) std::memcpy(pb + o_knot, knot_step, sizeof(int32_t) * kn);
    if (!h->st.cls_ints.empty()) std::memcpy(pb + o_cls, h->st.cls_ints.data(), sizeof(int32_t) * h->st.cls_ints.size());
    const double *pos = reinterpret_cast<const double *>(ag.blob.data());
    const double *vel = reinterpret_cast<const double *>(ag.blob.data() + ag.ao_vel);
    const sfw_agent_const *cst = reinterpret_cast<const sfw_agent_const *>(ag.blob.data() + ag.ao_cst);
    h->st.rest_pairs.clear();
    if (rest) {
      h->st.rest_pairs = ag.rest_pairs;
      h->st.rest_pv.assign(pos, pos + 2 * ag.A);
      h->st.rest_pv.insert(h->st.rest_pv.end(), vel, vel + 2 * ag.A);
      rest_forces(h->live.params, ag.rest_pairs, pos, vel, ag.A, reinterpret_cast<double *>(pb + o_rest));
    }
    const bool pinned = o_cls > o_pin && pinned_rest_table(h->live.params, *rs, pos, cst, ag.A, reinterpret_cast<double *>(pb + o_pin));
    ph.mark("pack");
    {
      const size_t from = send_cells ? 0 : cells_head;
      // A control cycle's grid whose costmap has not changed: no copy here.  If the launch turns out to be the one-launch kernel
      // its blocks read the (~1 KB) arena from this pinned memory themselves; else the launch enqueues the copy (flush_arena).
      // ... and a GPU-filling single-chunk grid: the pose rollout this stage enqueues below (plan_tables_device) fetches the
      // arena — with a small costmap that has changed, if any — itself, its thousands of threads 16 bytes each
      const int64_t T_ = static_cast<int64_t>(nv) * nw;
      const bool small = T_ <= 1024 && from == cells_head && total - from <= (size_t(16) << 10);
      const bool early = T_ > 2048 && chunk >= T_ && total - from <= (size_t(1) << 20);
      if (dev) {
        // The knot regions [o_lin, o_knot) hold nothing on the host: the copy goes around them, and the kernel that fills them
        // on the device is enqueued behind it (below).  Never pending: a kernel that fetched the arena from pinned memory
        // would read its sample vectors there.
        if (o_lin > from) SFW_HIP(h, hipMemcpyAsync(h->arena.p + from, pb + from, o_lin - from, hipMemcpyHostToDevice, h->stream));
        if (total > o_knot) SFW_HIP(h, hipMemcpyAsync(h->arena.p + o_knot, pb + o_knot, total - o_knot, hipMemcpyHostToDevice, h->stream));
      } else if (h->cfg.arena_direct_on && (small || early) && (total - from) % 16 == 0 && from % 16 == 0) {
        h->st.arena_pending = true;
        h->st.arena_from = from;
        h->st.arena_bytes = total - from;
      } else {
        SFW_HIP(h, hipMemcpyAsync(h->arena.p + from, pb + from, total - from, hipMemcpyHostToDevice, h->stream));
      }
    }
    h->st.d_cells = merge ? reinterpret_cast<const uint8_t *>(h->arena.p) : h->cells.p;
    ph.mark("h2d");
    if (!h->st.arena_pending) SFW_HIP(h, h->pin_arena.mark(h->stream));
    ph.mark("evrec");
    const char *db = h->arena.p;
    h->st.d_cls_tab = h->st.cls_ints.empty() ? nullptr : reinterpret_cast<const int32_t *>(db + o_cls);
    h->st.d_pin_rest = pinned ? reinterpret_cast<const double *>(db + o_pin) : nullptr;
    h->st.pin_doubles = pinned ? pin_doubles : 0;
    if (pinned) {
      h->st.pin_pos.assign(pos, pos + 2 * ag.A);
      h->st.pin_cst.assign(cst, cst + ag.A);
    }
    h->st.d_footprint = reinterpret_cast<const double *>(db + o_fp);
    h->st.d_agent_pos = reinterpret_cast<const double *>(db + o_ag);
    h->st.d_agent_vel = reinterpret_cast<const double *>(db + o_ag + ag.ao_vel);
    h->st.d_agent_c = reinterpret_cast<const sfw_agent_const *>(db + o_ag + ag.ao_cst);
    h->st.d_obstacles = reinterpret_cast<const double *>(db + o_ag + ag.ao_obs);
    h->st.d_agent_grp = reinterpret_cast<const int32_t *>(db + o_ag + ag.ao_grp);
    h->st.d_grp_off = reinterpret_cast<const int32_t *>(db + o_ag + ag.ao_off);
    h->st.d_grp_mem = reinterpret_cast<const int32_t *>(db + o_ag + ag.ao_mem);
    h->st.d_linvels = reinterpret_cast<const double *>(db + o_lin);
    h->st.d_angvels = reinterpret_cast<const double *>(db + o_ang);
    h->st.d_vy = has_vy ? reinterpret_cast<const double *>(db + o_vy) : nullptr;
    h->st.d_knot_step = knot_step ? reinterpret_cast<const int32_t *>(db + o_knot) : nullptr;
    h->st.d_agent_rest = rest ? reinterpret_cast<const double *>(db + o_rest) : nullptr;
  }
  if (h->pair_tab_A != ag.A) {
    h->pair_tab_A = -1;  // (until the table for this count is enqueued)
    SFW_HIP(h, h->pair_tab.reserve(static_cast<size_t>(sfw_pair_table_entries(ag.A))));
    SFW_HIP(h, sfw_launch_pair_table(h->pair_tab.p, ag.A, h->stream));
    h->pair_tab_A = ag.A;
  }
  const int64_t T = static_cast<int64_t>(nv) * nw;
  SFW_HIP(h, h->status.reserve(T));
  SFW_HIP(h, h->coll_step.reserve(T));
  SFW_HIP(h, h->base_cost.reserve(T));
  SFW_HIP(h, h->costs.reserve(T + (sizeof(sfw_sel) + sizeof(double) - 1) / sizeof(double)));
  h->st.d_sel = reinterpret_cast<sfw_sel *>(h->costs.p + T);
  SFW_HIP(h, h->partials.reserve(sfw_argmin_partials(T)));
  ph.mark("reserve");
  if (dev) {  // the knots, before anything that reads them (plan_tables_device may enqueue the pose rollout)
    double *z = nullptr;
    if (dev->keep_normals) {
      SFW_HIP(h, h->normals.reserve(3 * kn * static_cast<size_t>(nv)));
      z = h->normals.p;
    }
    SFW_HIP(h, sfw_launch_perturb(dev->args, nv, static_cast<int>(kn), index_base, const_cast<double *>(h->st.d_linvels),
                                  const_cast<double *>(h->st.d_vy), const_cast<double *>(h->st.d_angvels), z, h->stream));
    h->st.normals_kept = dev->keep_normals;
    ph.mark("perturb");
  }
  if (int e = plan_tables_device(h, chunk, true)) return e;
  if (T > 1024)
    if (int e = flush_arena(h)) return e;  // (no pose rollout was enqueued after all: the copy it would have stood in for)
  ph.mark("tables+K1a");
  stage_clearance(h, T);
  ph.mark("clearance");
  // commit: everything the arena carries is enqueued (a pending arena never carries cells: `small` keeps the head)
  if (merge) {
    h->world.cells_dirty = false;
    h->st.cells_in_arena = true;
    h->st.arena_cells_bytes = cells_head;
  }
  h->st.valid = true;
  return SFW_OK;
}

// The arena a stage left in pinned memory only (arena_pending) goes to the device by a copy after all: the launch is not the
// one-launch kernel, or something is about to patch the device copy.  A copy that cannot be enqueued leaves the device
// without the staged world: nothing is staged any more.
int flush_arena(sfw_handle h) {
  if (!h->st.arena_pending) return SFW_OK;
  h->st.arena_pending = false;
  hipError_t e = hipMemcpyAsync(h->arena.p + h->st.arena_from, h->pin_arena.p + h->st.arena_from, h->st.arena_bytes,
                                hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = h->pin_arena.mark(h->stream);
  if (e != hipSuccess) {
    drop_stage(h);
    return hip_fail(h, e, "flush_arena: arena copy");
  }
  return SFW_OK;
}

// What a launch of the staged grid settled before it enqueues its kernels (launch_prepare), for the two ways on: the one-kernel
// control cycle (cycle_launch_of -> the cycle kernel, alone or in a batch -> cycle_commit) or the kernels one by one
// (launch_kernels).
struct launch_prep {
  int64_t T = 0, chunk = 0;
  int S = 0;
  bool prefix = false, poses_done = false, single = false, timing = false;
  char *cap_pts = nullptr, *cap_n = nullptr, *cap_coll = nullptr;
  double *costs_host = nullptr;
  sfw_sel *sel_host = nullptr;
  double *terms = nullptr;  // sfw_set_terms_capture: the terms buffer, else null
};

// timing: record the per-kernel events of this launch (h->live.timing; a batch launch never does)
int launch_prepare(sfw_handle h, bool timing, launch_prep &lp) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!h->st.valid) return fail(h, SFW_ERR_STATE, "grid_launch before grid_stage");
  drop_launch(h);  // (launched again at the end of cycle_commit / launch_kernels, and only there)
  SFW_HIP(h, hipSetDevice(h->device));
  const int64_t T = static_cast<int64_t>(h->st.nv) * h->st.nw;
  // sfw_set_params since the stage: tables and shared-prefix plan are redone for the live parameters
  if (h->st.plan_epoch != h->live.params_epoch)
    if (int e = replan_at_launch(h)) {
      drop_stage(h);  // (a plan half redone fits neither parameter set)
      return e;
    }
  const int S = num_steps_of(h->live.params);
  int64_t chunk = h->st.table_chunk;  // (plan_tables_device: what the tables were sized for, under the live step count)
  if (chunk > kRowLimit) chunk = kRowLimit;
  if (chunk > T) chunk = T;
  if (chunk < 1) return fail(h, SFW_ERR_STATE, "robot-step table too small");
  if (int e = check_lds(h, h->st.A, h->st.O, h->st.NG, h->st.n_grp_mem, chunk)) return e;
  // the shared-prefix plan was laid out for the staged step count and for chunks of whole rows
  const bool prefix = !h->st.prefix_steps.empty() && h->st.prefix_S == S && h->st.prefix_chunk <= chunk;
  if (prefix) chunk = h->st.prefix_chunk;
  // the stage enqueued K1a of this (single-chunk) grid already — unless sfw_set_timing(1) arrived since: the events of a
  // timed launch bracket its own kernels, so the pose rollout runs again behind a freshly recorded ev[0]
  const bool poses_done = h->st.early_poses && chunk >= T && (!timing || h->st.early_poses_timed) &&
                          (!h->live.capture_terms || h->st.early_poses_terms);  // (capture turned on since the stage: roll out again)
  h->st.early_poses = false;                                 // ... once: a second launch of the same stage rolls out again
  if (timing) {
    SFW_HIP(h, h->clock.reserve(4));
    // (cleared by the stage already when it started the pose rollout: in front of it, where the GPU waits for the host's
    // planning anyway, instead of between the rollout and the first K2 dispatch)
    // ... or will be by the pose rollout this launch enqueues; only the small-grid kernels (a block per sample, no kernel in
    // front of their K2 part) need the memset
    if (!(poses_done && h->st.clock_cleared) && sfw_rollout_is_fused(std::min<int64_t>(T, chunk), S))
      SFW_HIP(h, hipMemsetAsync(h->clock.p, 0, 4 * sizeof(unsigned long long), h->stream));
    if (!poses_done) SFW_HIP(h, hipEventRecord(h->ev[0], h->stream));
  }
  h->st.clock_cleared = false;
  const bool single = chunk >= T;
  h->last.n_chunks = static_cast<int>((T + chunk - 1) / chunk);
  if (!single && timing) {
    while (h->chunk_ev.size() < static_cast<size_t>(3 * h->last.n_chunks)) {
      hipEvent_t e = nullptr;
      SFW_HIP(h, hipEventCreate(&e));
      h->chunk_ev.push_back(e);
    }
  }
  // Trajectory points on request (sfw_set_points_capture), when the whole grid goes through the fused K1
  char *cap_pts = nullptr, *cap_n = nullptr, *cap_coll = nullptr;
  if (h->live.capture_points && single) {
    if (sfw_rollout_is_fused(T, S)) {
      const size_t pts_bytes = sizeof(double) * 3 * static_cast<size_t>(S) * static_cast<size_t>(T);
      // (in pinned HOST memory: the kernels write points, counts and contact steps over PCIe as they go — 43 KB for 45 samples
      // of 40 steps — and the dump is a memcpy; until round 5 a device buffer and a D2H copy per dump, 12 us)
      if (pts_bytes + 8 * static_cast<size_t>(T) > h->pin_cap.cap) SFW_HIP(h, hipStreamSynchronize(h->stream));
      SFW_HIP(h, h->pin_cap.reserve(pts_bytes + 8 * static_cast<size_t>(T)));
      cap_pts = h->pin_cap.p;
      cap_n = cap_pts + pts_bytes;
      cap_coll = cap_n + 4 * static_cast<size_t>(T);
      h->last.captured = true;
      h->last.cap_S = S;
    }
  }
  // the cost vector and the selection record reach the host through the selection kernels themselves (pinned mirror): the
  // fetch then only waits for the stream.  Grids whose vector is larger than SFW_MIRROR_MAX_MB (default 64) keep the copy.
  double *costs_host = nullptr;
  sfw_sel *sel_host = nullptr;
  if (h->cfg.mirror_max_bytes > 0 && sizeof(double) * static_cast<size_t>(T) <= h->cfg.mirror_max_bytes) {
    const size_t cost_bytes = sizeof(double) * static_cast<size_t>(T);
    // (growing it frees the old area: no launch still in the stream may be writing there)
    if (cost_bytes + sizeof(sfw_sel) > h->pin_mirror.cap) SFW_HIP(h, hipStreamSynchronize(h->stream));
    SFW_HIP(h, h->pin_mirror.reserve(cost_bytes + sizeof(sfw_sel)));
    costs_host = reinterpret_cast<double *>(h->pin_mirror.p);
    sel_host = reinterpret_cast<sfw_sel *>(h->pin_mirror.p + cost_bytes);
    h->last.mirrored = true;
  }
  lp.T = T;
  lp.chunk = chunk;
  lp.S = S;
  lp.prefix = prefix;
  lp.poses_done = poses_done;
  lp.single = single;
  lp.timing = timing;
  lp.cap_pts = cap_pts;
  lp.cap_n = cap_n;
  lp.cap_coll = cap_coll;
  lp.costs_host = costs_host;
  lp.sel_host = sel_host;
  if (h->live.capture_terms) {
    SFW_HIP(h, h->terms.reserve(static_cast<size_t>(SFW_N_TERMS) * static_cast<size_t>(T)));
    lp.terms = h->terms.p;
    h->last.terms = true;
  }
  return SFW_OK;
}

// What a launch record of the staged grid writes beside the handle's own per-sample buffers: the captured points, the clock
// probe of a timed launch, the captured terms
void bind_launch_outputs(sfw_handle h, const launch_prep &lp, sfw_launch &L) {
  if (h->last.captured) {
    L.points = reinterpret_cast<double *>(lp.cap_pts);
    L.n_points = reinterpret_cast<int32_t *>(lp.cap_n);
    L.coll_step = reinterpret_cast<int32_t *>(lp.cap_coll);
    // a sample the costmap rejects at pose a may touch a pedestrian at an earlier step b < a, where the reference's
    // Trajectory ends (ref :613-627): integrated all the same, its cost stays -1 (finish_wave)
    L.force_alive = 1;
  }
  L.clock_probe = lp.timing ? h->clock.p : nullptr;  // every K2 dispatch writes it; the last one (the launch over the samples) stays
  L.terms = lp.terms;
  L.terms_T = lp.T;
}

// A control cycle's grid: K1 + K2 + K3 in ONE launch (sfw_cycle_kernel) when the launch qualifies.  Step 1: the launch record
// (false: it does not qualify; nothing has changed).
bool cycle_launch_of(sfw_handle h, const launch_prep &lp, sfw_launch &L) {
  if (!(lp.single && !lp.prefix && !lp.poses_done)) return false;
  fill_launch(h, L, 0, lp.T, lp.chunk);
  bind_launch_outputs(h, lp, L);
  L.costs_host = lp.costs_host;
  L.sel_host = lp.sel_host;
  if (!sfw_cycle_applies(L)) return false;
  arena_by_kernel(h, L);  // no copy at all this cycle
  return true;
}
// Step 2, once the kernel that carries L is enqueued: the handle's state after its launch
int cycle_commit(sfw_handle h, bool timing) {
  SFW_HIP(h, arena_fetched(h));
  if (timing) {
    SFW_HIP(h, hipEventRecord(h->ev[2], h->stream));
    SFW_HIP(h, hipEventRecord(h->ev[3], h->stream));
  }
  h->last.timed = timing;
  h->last.cycle = true;
  ++h->launch_seq;
  h->last.launched = true;
  return SFW_OK;
}

// Everything else: K1, K2 and the selection as kernels of their own (chunks, shared-prefix levels)
int launch_kernels(sfw_handle h, const launch_prep &lp) {
  const int64_t T = lp.T, chunk = lp.chunk;
  const int S = lp.S;
  const bool prefix = lp.prefix, poses_done = lp.poses_done, single = lp.single, timing = lp.timing;
  double *const costs_host = lp.costs_host;
  sfw_sel *const sel_host = lp.sel_host;
  if (int e = flush_arena(h)) return e;
  int c = 0;
  for (int64_t b = 0; b < T; b += chunk, ++c) {
    const int64_t n = (T - b < chunk) ? (T - b) : chunk;
    sfw_launch L;
    fill_launch(h, L, b, n, chunk);
    bind_launch_outputs(h, lp, L);
    if (!single && timing) SFW_HIP(h, hipEventRecord(h->chunk_ev[3 * c], h->stream));
    if (prefix) {
      // K1a -> { K2 prefix phase on the main stream  ||  K1b + K1c on the side stream } -> K2 suffix phase.
      // The prefix phase needs the robot-step table only and under-fills the GPU (one item per class).
      // The levels are the critical path and are enqueued FIRST; the footprint checks only have to be done when the suffix
      // launch starts, so their stream gets its work afterwards (enqueued in front of the levels — round 4 — the four
      // side-stream calls delayed the first level by the host time they take: ~15 us of cfg2's 630 us step).
      if (!poses_done) SFW_HIP(h, sfw_launch_rollout_poses(L, h->stream));
      SFW_HIP(h, hipEventRecord(h->ev_poses, h->stream));
      if (timing) SFW_HIP(h, hipEventRecord(single ? h->ev[1] : h->chunk_ev[3 * c + 1], h->stream));
      const chunk_plan &cp = h->st.prefix_chunks[static_cast<size_t>(c)];
      const int32_t *tab = h->st.d_cls_tab;
      const size_t n_lv = h->st.prefix_steps.size();
      for (size_t l = 0; l < n_lv; ++l) {  // the tree of shared steps, coarsest classes first
        const level_tables &t = cp.lv[l];
        L.phase = SFW_PHASE_PREFIX;
        L.step_begin = l ? h->st.prefix_steps[l - 1] : 0;
        L.step_end = h->st.prefix_steps[l];
        L.n_cls = t.n_row * t.n_col;
        L.n_col_cls = t.n_col;
        L.row_rep = tab + t.o_row_rep;
        L.col_rep = tab + t.o_col_rep;
        L.resume = l > 0;
        if (l > 0) {
          L.n_col_src = cp.lv[l - 1].n_col;
          L.row_src = tab + t.o_row_src;
          L.col_src = tab + t.o_col_src;
          L.in_state = h->cls_state[(l - 1) & 1].p;
          L.in_dead = h->cls_dead[(l - 1) & 1].p;
        }
        L.out_state = h->cls_state[l & 1].p;
        L.out_dead = h->cls_dead[l & 1].p;
        SFW_HIP(h, launch_social_of(L, h->stream));
      }
      {  // K1b + K1c beside the levels (they wait for the pose rollout, not for the levels)
        sfw_launch Lc = L;
        Lc.phase = SFW_PHASE_WHOLE;
        SFW_HIP(h, hipStreamWaitEvent(h->side, h->ev_poses, 0));
        SFW_HIP(h, sfw_launch_rollout_costmap(Lc, h->side));
        SFW_HIP(h, hipEventRecord(h->ev_side, h->side));
      }
      SFW_HIP(h, hipStreamWaitEvent(h->stream, h->ev_side, 0));
      L.phase = SFW_PHASE_SUFFIX;
      L.step_begin = h->st.prefix_steps.back();
      L.step_end = S;
      L.resume = 1;
      L.n_col_src = cp.lv[n_lv - 1].n_col;
      L.row_src = tab + cp.o_row_cls;
      L.col_src = tab + h->st.prefix_o_col_cls;
      L.in_state = h->cls_state[(n_lv - 1) & 1].p;
      L.in_dead = h->cls_dead[(n_lv - 1) & 1].p;
      SFW_HIP(h, launch_social_of(L, h->stream, &h->split));  // (`side` is idle: the stream has just waited for it)
    } else {
      if (!poses_done) SFW_HIP(h, sfw_launch_rollout_poses(L, h->stream));
      SFW_HIP(h, sfw_launch_rollout_costmap(L, h->stream));
      if (timing) SFW_HIP(h, hipEventRecord(single ? h->ev[1] : h->chunk_ev[3 * c + 1], h->stream));
      SFW_HIP(h, launch_social_of(L, h->stream, &h->split));
    }
    // sfw_set_path: cost + w p behind whatever formed the chunk's costs, in front of the selection
    if (L.path_on) SFW_HIP(h, sfw_launch_path_add(L.costs, L.path_p, h->st.path_weight, b, n, h->stream));
    if (!single && timing) SFW_HIP(h, hipEventRecord(h->chunk_ev[3 * c + 2], h->stream));
  }
  if (timing) SFW_HIP(h, hipEventRecord(h->ev[2], h->stream));
  SFW_HIP(h, sfw_launch_argmin(h->costs.p, h->st.d_linvels, h->st.d_angvels, h->st.nw, T, h->st.index_base,
                               h->partials.p, h->st.d_sel, h->stream, costs_host, sel_host, h->st.list));
  if (timing) SFW_HIP(h, hipEventRecord(h->ev[3], h->stream));
  h->last.timed = timing;
  ++h->launch_seq;
  h->last.launched = true;
  return SFW_OK;
}

hipError_t launch_cycle_of(const sfw_launch &L, hipStream_t stream) {
  return L.p.precision == SFW_PRECISION_F64_STRICT ? sfw_launch_cycle_strict(L, stream) : sfw_launch_cycle(L, stream);
}

int launch_common(sfw_handle h) {
  launch_prep lp;
  if (int e = launch_prepare(h, h ? h->live.timing : false, lp)) return e;
  sfw_launch L;
  if (cycle_launch_of(h, lp, L)) {
    if (lp.timing) SFW_HIP(h, hipEventRecord(h->ev[1], h->stream));  // (no K1 of its own: K1 time 0, the launch is "K2")
    SFW_HIP(h, launch_cycle_of(L, h->stream));
    return cycle_commit(h, lp.timing);
  }
  return launch_kernels(h, lp);
}

// Knots of samples [first, first + count) of a stage whose knots the device holds, into pin_knots: rows[c][k * count + i] for
// the channels c the stage has (vy: null without a vy vector), behind everything enqueued on the stream.  Waits for the stream.
int knots_from_device(sfw_handle h, int64_t first, int64_t count, const double *rows[3]) {
  const size_t K = static_cast<size_t>(h->st.nk), row = sizeof(double) * static_cast<size_t>(count);
  SFW_HIP(h, hipSetDevice(h->device));
  if (3 * K * row > h->pin_knots.cap) SFW_HIP(h, hipStreamSynchronize(h->stream));  // (growing the area frees the old one)
  SFW_HIP(h, h->pin_knots.reserve(3 * K * row));
  const double *src[3] = {h->st.d_linvels, h->st.d_vy, h->st.d_angvels};
  for (int c = 0; c < 3; ++c) {
    rows[c] = nullptr;
    if (!src[c]) continue;
    char *dst = h->pin_knots.p + static_cast<size_t>(c) * K * row;
    SFW_HIP(h, hipMemcpy2DAsync(dst, row, src[c] + first, sizeof(double) * static_cast<size_t>(h->st.nv), row, K, hipMemcpyDeviceToHost,
                                h->stream));
    rows[c] = reinterpret_cast<const double *>(dst);
  }
  SFW_HIP(h, wait_stream(h));
  return SFW_OK;
}

int sel_to_best(sfw_handle h, const sfw_sel &s, sfw_best *best, sfw_best_key *key) {
  const bool found = std::isfinite(s.cost);
  if (best) {
    best->n_valid = s.n_valid;
    if (found) {
      const int64_t local = -s.neg_index - h->st.index_base;
      best->index = local;
      best->cost = s.cost;
      if (h->st.perturbed) {  // the winner's first knot, from the device: the host holds no knots of a perturbed stage
        const double *rows[3];
        if (int e = knots_from_device(h, local, 1, rows)) return e;
        best->vx = rows[0][0];
        best->vy = rows[1] ? rows[1][0] : 0.0;
        best->vtheta = rows[2][0];
      } else if (h->st.list) {  // the sample's own three values
        best->vx = h->st.lin[static_cast<size_t>(local)];
        best->vy = h->st.vy.empty() ? 0.0 : h->st.vy[static_cast<size_t>(local)];
        best->vtheta = h->st.ang[static_cast<size_t>(local)];
      } else {
        best->vx = h->st.lin[static_cast<size_t>(local / h->st.nw)];
        best->vy = 0.0;
        best->vtheta = h->st.ang[static_cast<size_t>(local % h->st.nw)];
      }
    } else {  // ref :456-468: stop the robot
      best->index = -1;
      best->cost = -1.0;
      best->vx = best->vy = best->vtheta = 0.0;
    }
  }
  if (key) {
    key->cost = found ? s.cost : std::numeric_limits<double>::infinity();
    key->neg_linvel = found ? s.neg_linvel : std::numeric_limits<double>::infinity();
    key->abs_angvel = found ? s.abs_angvel : std::numeric_limits<double>::infinity();
    key->neg_index = found ? static_cast<double>(s.neg_index) : std::numeric_limits<double>::infinity();
  }
  return SFW_OK;
}

// The argument rules of the sequence stages as texts of their own: null when the arguments are accepted, else why not.  The
// handle's stages and the ensemble's score calls (which must refuse before ANY member is staged) read the same ones.
const char *sequences_refusal(int32_t K, const int32_t *knot_step) {
  if (K < 1 || K > SFW_SEQ_MAX_KNOTS) return "K outside 1..SFW_SEQ_MAX_KNOTS";
  if (!knot_step) return "knot_step is NULL";
  if (knot_step[0] != 0) return "knot_step[0] must be 0";
  for (int32_t k = 1; k < K; ++k)
    if (knot_step[k] <= knot_step[k - 1]) return "knot_step must be strictly ascending";
  return nullptr;
}
const char *perturb_refusal(const sfw_robot_state *rs, const sfw_perturb *p, int32_t n, int32_t K, const int32_t *knot_step,
                            const sfw_goal_args *args, int64_t index_base) {
  if (!rs || !p || !p->nominal || !knot_step || !args) return "rs, p, p->nominal, knot_step or args is NULL";
  if (n < 1) return "n < 1";
  if (const char *why = sequences_refusal(K, knot_step)) return why;
  if (index_base < 0) return "index_base < 0";
  constexpr int32_t known = SFW_PERTURB_KEEP_NOMINAL | SFW_PERTURB_NO_VY | SFW_PERTURB_KEEP_NORMALS;
  if ((p->flags & ~known) != 0 || p->reserved != 0) return "unknown flag bits, or reserved != 0";
  if (!all_finite(p->nominal, 3 * static_cast<size_t>(K)) || !all_finite(p->sigma, 3) || !all_finite(p->lo, 3) || !all_finite(p->hi, 3))
    return "non-finite nominal, sigma, lo or hi";
  for (int c = 0; c < 3; ++c) {
    if (p->sigma[c] < 0.0) return "a sigma is negative";
    if (p->lo[c] > p->hi[c]) return "lo > hi";
  }
  if ((p->flags & SFW_PERTURB_NO_VY) != 0) {
    if (p->sigma[1] != 0.0) return "SFW_PERTURB_NO_VY with sigma[1] != 0";
    for (int32_t k = 0; k < K; ++k)
      if (p->nominal[3 * k + 1] != 0.0) return "SFW_PERTURB_NO_VY with a nominal vy != 0";
  }
  return nullptr;
}
// ... and stage_common's own (stage_null_refusal, stage_finite_refusal) for the list a request describes
const char *list_stage_refusal(const sfw_robot_state *rs, const sfw_goal_args *args, const stage_request &q) {
  if (const char *why = stage_null_refusal(rs, args, q)) return why;
  return stage_finite_refusal(rs, args, q);
}
const char *blend_refusal(const double *lambda, int32_t L, const sfw_blend_stat *stat_out, const double *u_out) {
  if (!lambda || !stat_out || !u_out) return "lambda, stat_out or u_out is NULL";
  if (L < 1 || L > SFW_BLEND_MAX_L) return "L out of [1, SFW_BLEND_MAX_L]";
  for (int32_t l = 0; l < L; ++l)
    if (!std::isfinite(lambda[l]) || !(lambda[l] > 0.0)) return "a lambda is not finite or not > 0";
  return nullptr;
}

// The softmin blend over a device cost vector of T samples, on h's stream and into the buffers `a` (h's own; an sfw_ensemble's):
// ONE text for sfw_grid_blend and sfw_ensemble_blend.  The knot rows are those of h's stage: st.nk rows (1: a grid, a plain list)
// at st.d_linvels / d_vy / d_angvels.  Arguments and state are the caller's to check.
//
// What a blend leaves in pinned memory (a "slot"): the minimum record | eta[L] | sum_w2[L] | u[L][K][3]
constexpr size_t kBlendHead = (sizeof(sfw_blend_min) + 15) & ~size_t(15);
size_t blend_slot_bytes(int L, int K) { return kBlendHead + sizeof(double) * static_cast<size_t>(sfw_blend_channels(L, K)); }

// The blend in two parts.  blend_enqueue: the kernels (and the copies of weights_out) on h's stream, no wait — d_bias
// (nullable) is ON THE DEVICE and `slot` is pinned memory of blend_slot_bytes(L, st.nk) that stays put until the stream has been
// waited for.  plan (sfw_mppi_run, L == 1): see sfw_launch_blend.  blend_finish: the outputs from a slot the stream is done with.
int blend_enqueue(sfw_handle h, blend_buffers &a, const double *d_costs, int64_t T, const double *lambda, int32_t L, const double *d_bias,
                  double *weights_out, char *slot, double *plan = nullptr) {
  const int K = h->st.nk;
  const int64_t n_ch = sfw_blend_channels(L, K), blocks = sfw_blend_blocks(T);
  SFW_HIP(h, a.mins.reserve(static_cast<size_t>(sfw_blend_min_blocks(T))));
  SFW_HIP(h, a.partials.reserve(static_cast<size_t>(blocks) * static_cast<size_t>(n_ch)));
  // weights_out: all L vectors from the launch that forms the sums, or — beyond 256 MB of them — in slices of as many
  // temperatures as that holds, each by a launch of its own that is copied out behind it
  const int64_t fit = std::max<int64_t>(1, (int64_t(256) << 20) / (static_cast<int64_t>(sizeof(double)) * T));
  const bool sliced = weights_out && fit < L;
  const int32_t l_step = static_cast<int32_t>(std::min<int64_t>(L, fit));
  if (weights_out) SFW_HIP(h, a.weights.reserve(static_cast<size_t>(l_step) * static_cast<size_t>(T)));
  sfw_blend_lambdas lam{};
  for (int32_t l = 0; l < L; ++l) lam.v[l] = lambda[l];
  sfw_blend_min *const min_host = reinterpret_cast<sfw_blend_min *>(slot);
  double *const out_host = reinterpret_cast<double *>(slot + kBlendHead);
  SFW_HIP(h, sfw_launch_blend(d_costs, d_bias, T, lam, L, K, h->st.d_linvels, h->st.d_vy, h->st.d_angvels, h->st.nw, h->st.list, a.mins.p, a.partials.p,
                              weights_out && !sliced ? a.weights.p : nullptr, min_host, out_host, h->stream, plan));
  if (weights_out && !sliced)
    SFW_HIP(h, hipMemcpyAsync(weights_out, a.weights.p, sizeof(double) * static_cast<size_t>(L) * static_cast<size_t>(T),
                              hipMemcpyDeviceToHost, h->stream));
  for (int32_t l0 = 0; sliced && l0 < L; l0 += l_step) {
    const int32_t n = std::min(l_step, L - l0);
    sfw_blend_lambdas part{};
    for (int32_t l = 0; l < n; ++l) part.v[l] = lambda[l0 + l];
    SFW_HIP(h, sfw_launch_blend_weights(d_costs, d_bias, T, part, n, a.mins.p, a.weights.p, h->stream));
    SFW_HIP(h, hipMemcpyAsync(weights_out + static_cast<int64_t>(l0) * T, a.weights.p,
                              sizeof(double) * static_cast<size_t>(n) * static_cast<size_t>(T), hipMemcpyDeviceToHost, h->stream));
  }
  return SFW_OK;
}
void blend_finish(const char *slot, const double *lambda, int32_t L, int K, sfw_blend_stat *stat_out, double *u_out) {
  sfw_blend_min m;
  std::memcpy(&m, slot, sizeof(m));
  const double *const out_host = reinterpret_cast<const double *>(slot + kBlendHead);
  const bool any = m.n_valid > 0;
  for (int32_t l = 0; l < L; ++l) {
    stat_out[l].lambda = lambda[l];
    stat_out[l].j_min = any ? m.j : -1.0;
    stat_out[l].eta = out_host[l];
    stat_out[l].sum_w2 = out_host[L + l];
    stat_out[l].n_valid = m.n_valid;
    stat_out[l].index_min = any ? m.index : -1;
  }
  std::memcpy(u_out, out_host + 2 * L, sizeof(double) * 3 * static_cast<size_t>(K) * static_cast<size_t>(L));
}
// The blocking blend: the area's pinned slot, the enqueue, one wait, the finish.  bias (nullable, host) goes up first; d_bias
// (nullable) is a bias vector the device holds already, read instead.
int blend_run(sfw_handle h, blend_buffers &a, const double *d_costs, int64_t T, const double *lambda, int32_t L, const double *bias,
              sfw_blend_stat *stat_out, double *u_out, double *weights_out, const double *d_bias) {
  const int K = h->st.nk;
  const size_t out_bytes = blend_slot_bytes(L, K);
  // (growing the pinned area frees the old one: nothing in the stream may still be writing there)
  if (out_bytes > a.pin.cap) SFW_HIP(h, hipStreamSynchronize(h->stream));
  SFW_HIP(h, a.pin.reserve(out_bytes));
  if (bias) {
    SFW_HIP(h, a.bias.reserve(static_cast<size_t>(T)));
    SFW_HIP(h, hipMemcpyAsync(a.bias.p, bias, sizeof(double) * static_cast<size_t>(T), hipMemcpyHostToDevice, h->stream));
    d_bias = a.bias.p;
  }
  if (int e = blend_enqueue(h, a, d_costs, T, lambda, L, d_bias, weights_out, a.pin.p)) return e;
  SFW_HIP(h, a.pin.mark(h->stream));
  SFW_HIP(h, wait_stream(h));
  a.pin.pending = false;
  blend_finish(a.pin.p, lambda, L, K, stat_out, u_out);
  return SFW_OK;
}

// The bias vector gamma * c_t (+ bias[t], nullable: T host doubles, uploaded to the blend's bias buffer first) of the staged
// perturbed stage into mb.ctrl_bias, on h's stream.  plan (nullable): the nominal rows in device memory (sfw_mppi_run).  mb / bb:
// the handle's buffers, or an sfw_ensemble's own (member 0's belong to that member's calls).
int control_cost_enqueue(sfw_handle h, double gamma, const double *bias, const double *plan, mppi_buffers &mb, blend_buffers &bb) {
  dev_buf<double> &out = mb.ctrl_bias, &add = bb.bias;
  const int64_t n = h->st.nv;
  SFW_HIP(h, out.reserve(static_cast<size_t>(n)));
  const double *d_add = nullptr;
  if (bias) {
    SFW_HIP(h, add.reserve(static_cast<size_t>(n)));
    SFW_HIP(h, hipMemcpyAsync(add.p, bias, sizeof(double) * static_cast<size_t>(n), hipMemcpyHostToDevice, h->stream));
    d_add = add.p;
  }
  SFW_HIP(h, sfw_launch_control_cost(h->st.pert, plan, h->st.nk, n, h->st.index_base, h->st.normals_kept ? h->normals.p : nullptr, gamma,
                                     d_add, out.p, h->stream));
  return SFW_OK;
}
const char *control_state_refusal(sfw_handle h) {
  return h->st.valid && h->st.perturbed ? nullptr : "no perturbed stage (sfw_sequences_perturb_stage, sfw_mppi_run) is staged";
}


// sfw_grid_blend (gamma null) and sfw_grid_blend_control over the last launch's cost vector: ONE text, the shape of
// ensemble_blend.  The control cost goes into the handle's ctrl_bias, on top of `bias` when there is one.
int grid_blend(sfw_handle h, const char *what, const double *lambda, int32_t L, const double *gamma, const double *bias,
               sfw_blend_stat *stat_out, double *u_out, double *weights_out) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (const char *why = blend_refusal(lambda, L, stat_out, u_out)) return fail(h, SFW_ERR_INVALID_ARG, std::string(what) + ": " + why);
  if (gamma && !std::isfinite(*gamma)) return fail(h, SFW_ERR_INVALID_ARG, std::string(what) + ": gamma is not finite");
  if (gamma)
    if (const char *why = control_state_refusal(h)) return fail(h, SFW_ERR_STATE, std::string(what) + ": " + why);
  if (!h->last.launched) return fail(h, SFW_ERR_STATE, std::string(what) + ": no launch, or a stage or sfw_score_one came in since");
  const int64_t T = static_cast<int64_t>(h->st.nv) * h->st.nw;
  if (bias && !all_finite(bias, static_cast<size_t>(T))) return fail(h, SFW_ERR_INVALID_ARG, std::string(what) + ": non-finite bias");
  SFW_HIP(h, hipSetDevice(h->device));
  // gamma == 0: sfw_grid_blend itself (a bias of gamma * c_t = +-0.0 would turn a cost of -0.0 into +0.0)
  const double *d_bias = nullptr;
  if (gamma && *gamma != 0.0) {
    if (int e = control_cost_enqueue(h, *gamma, bias, nullptr, h->mppi, h->blend)) return e;
    d_bias = h->mppi.ctrl_bias.p;
    bias = nullptr;
  }
  return blend_run(h, h->blend, h->costs.p, T, lambda, L, bias, stat_out, u_out, weights_out, d_bias);
}

// The sfw_mppi argument rules of sfw_mppi_run and sfw_ensemble_mppi_run (m null: the first one's to report; each call words its
// null pointers itself)
const char *const kMppiIterations = "iterations outside 1..SFW_MPPI_MAX_ITER, or reserved != 0";
const char *mppi_refusal(const sfw_mppi *m) {
  if (!m || m->iterations < 1 || m->iterations > SFW_MPPI_MAX_ITER || m->reserved != 0) return kMppiIterations;
  if (!std::isfinite(m->lambda) || !(m->lambda > 0.0) || !std::isfinite(m->gamma))
    return "lambda is not finite or not > 0, or gamma is not finite";
  return nullptr;
}

void perturb_seed(sfw_perturb_dev &d, uint64_t seed) {
  d.key0 = static_cast<uint32_t>(seed & 0xffffffffu);
  d.key1 = static_cast<uint32_t>(seed >> 32);
}

// The pinned area of a chain of I iterations with K knots: one blend slot per iteration | the caller's nominal | `extra` bytes
// (16-aligned: an ensemble's member table)
struct mppi_slots {
  size_t slot, plan_bytes, plan_at, extra_at, bytes;
  mppi_slots(int I, int K, size_t extra)
      : slot((blend_slot_bytes(1, K) + 15) & ~size_t(15)), plan_bytes(sizeof(double) * 3 * static_cast<size_t>(K)), plan_at(I * slot),
        extra_at((plan_at + plan_bytes + 15) & ~size_t(15)), bytes(extra ? extra_at + extra : plan_at + plan_bytes) {}
};
// Every buffer a chain over n samples writes is in place before its first kernel is enqueued: nothing in flight is ever freed.
// (A pinned area that has to grow frees the old one: the caller waits for its stream first.)
hipError_t mppi_reserve(mppi_buffers &mb, blend_buffers &bb, const mppi_slots &s, int K, int64_t n, bool control) {
  hipError_t e = mb.pin_mppi.reserve(s.bytes);
  if (e == hipSuccess) e = mb.mppi_plan.reserve(3 * static_cast<size_t>(SFW_SEQ_MAX_KNOTS));
  if (e == hipSuccess && control) e = mb.ctrl_bias.reserve(static_cast<size_t>(n));
  if (e == hipSuccess) e = bb.mins.reserve(static_cast<size_t>(sfw_blend_min_blocks(n)));
  if (e == hipSuccess) e = bb.partials.reserve(static_cast<size_t>(sfw_blend_blocks(n)) * static_cast<size_t>(sfw_blend_channels(1, K)));
  return e;
}
// After THE wait: every iteration's statistics and plan from its slot; and the stage each of the nh handles holds is iteration
// I - 1's, drawn around nom_(I-1)
void mppi_finish(const mppi_slots &s, const char *pin, const sfw_mppi *m, int K, sfw_blend_stat *stat_out, double *plans_out,
                 const sfw_handle *hs, size_t nh) {
  const int I = m->iterations;
  for (int i = 0; i < I; ++i) blend_finish(pin + i * s.slot, &m->lambda, 1, K, stat_out + i, plans_out + static_cast<size_t>(i) * 3 * K);
  if (I > 1)
    for (size_t k = 0; k < nh; ++k) std::memcpy(hs[k]->st.pert.nominal, plans_out + static_cast<size_t>(I - 2) * 3 * K, s.plan_bytes);
}

// sfw_mppi_run behind its stage of iteration 0: everything enqueued, one wait, the outputs.  A failure is the caller's to clean up.
int mppi_chain(sfw_handle h, const sfw_perturb *p, const sfw_mppi *m, sfw_blend_stat *stat_out, double *plans_out, sfw_best *best_out) {
  const int I = m->iterations, K = h->st.nk;
  const int64_t n = h->st.nv;
  const mppi_slots s(I, K, 0);
  SFW_HIP(h, hipSetDevice(h->device));
  if (s.bytes > h->mppi.pin_mppi.cap) SFW_HIP(h, hipStreamSynchronize(h->stream));
  SFW_HIP(h, mppi_reserve(h->mppi, h->blend, s, K, n, m->gamma != 0.0));
  char *const pin = h->mppi.pin_mppi.p;
  std::memcpy(pin + s.plan_at, p->nominal, s.plan_bytes);
  SFW_HIP(h, hipMemcpyAsync(h->mppi.mppi_plan.p, pin + s.plan_at, s.plan_bytes, hipMemcpyHostToDevice, h->stream));
  double *const plan = h->mppi.mppi_plan.p;
  for (int i = 0; i < I; ++i) {
    if (i > 0) {  // the stage of iteration i: its seed, and the knots drawn around the plan the last update left
      perturb_seed(h->st.pert, p->seed + static_cast<uint64_t>(i));
      SFW_HIP(h, sfw_launch_perturb_plan(h->st.pert, plan, n, K, 0, const_cast<double *>(h->st.d_linvels), const_cast<double *>(h->st.d_vy),
                                         const_cast<double *>(h->st.d_angvels), h->st.normals_kept ? h->normals.p : nullptr, h->stream));
    }
    if (int e = launch_common(h)) return e;
    const double *d_bias = nullptr;
    if (m->gamma != 0.0) {  // (as sfw_grid_blend_control: gamma == 0 is the plain blend)
      if (int e = control_cost_enqueue(h, m->gamma, nullptr, plan, h->mppi, h->blend)) return e;
      d_bias = h->mppi.ctrl_bias.p;
    }
    if (int e = blend_enqueue(h, h->blend, h->costs.p, n, &m->lambda, 1, d_bias, nullptr, pin + i * s.slot, plan)) return e;
  }
  SFW_HIP(h, h->mppi.pin_mppi.mark(h->stream));
  sfw_best best;
  if (int e = sfw_grid_fetch(h, nullptr, &best, nullptr)) return e;  // THE wait (and the winner's first knot behind it)
  h->mppi.pin_mppi.pending = false;
  mppi_finish(s, pin, m, K, stat_out, plans_out, &h, 1);
  if (best_out) *best_out = best;
  return SFW_OK;
}

// The blocking score behind its stage, whose status is `staged`: launch + fetch
int score_staged(sfw_handle h, int staged, double *costs_out, sfw_best *best_out) {
  if (staged) return staged;
  if (int e = sfw_grid_launch(h)) return e;
  return sfw_grid_fetch(h, costs_out, best_out, nullptr);
}

// The scratch set (rerun_buffers) for a re-run of `count` samples of the staged grid.  path: the re-run also forms the path
// term — crowd_run, whose cost carries the term; the re-runs that only want poses leave the term's kernels out.
hipError_t reserve_scratch(sfw_handle h, int64_t count, bool path) {
  rerun_buffers &b = h->pts;
  const size_t n = static_cast<size_t>(count), S = static_cast<size_t>(num_steps_of(h->live.params));
  hipError_t e = b.status.reserve(n);
  if (e == hipSuccess) e = b.coll.reserve(n);
  if (e == hipSuccess) e = b.base.reserve(n);
  if (e == hipSuccess) e = b.costs.reserve(n);
  if (e == hipSuccess) e = b.ptab.reserve(S * static_cast<size_t>(table_row_units(count, h->st.nw)));
  if (e == hipSuccess) e = b.cs.reserve(S * (h->st.list ? n : static_cast<size_t>(h->st.nw)));
  if (e == hipSuccess) e = b.fcode.reserve(S * n);
  if (h->st.stop_on) {
    if (e == hipSuccess) e = b.stop_steps.reserve(n);
    if (e == hipSuccess) e = b.stop_hit.reserve(n);
    if (e == hipSuccess) e = b.stop_tail.reserve(n * static_cast<size_t>(h->st.stop_cap));
  }
  if (h->st.path_on && path) {
    if (e == hipSuccess) e = b.path_p.reserve(n);
    if (e == hipSuccess) e = b.path_D.reserve(n * S);
  }
  return e;
}
// The launch record of samples [first, first + count) run once more, alone, into that set (reserve_scratch with the same count
// and path in front).  The kernels index per-sample outputs by the global sample index: the pointers are biased by -first.
// coll: the re-run's contact steps go to the set too (else nowhere: the launch's own are kept).
void fill_scratch_launch(sfw_handle h, sfw_launch &L, int64_t first, int64_t count, bool path, bool coll) {
  const rerun_buffers &b = h->pts;
  fill_launch(h, L, first, count, count);
  L.status = b.status.p - first;
  L.base_cost = b.base.p - first;
  L.costs = b.costs.p - first;
  L.coll_step = coll ? b.coll.p - first : nullptr;
  L.ptab = b.ptab.p;
  L.cs_tab = b.cs.p;
  L.fcode = b.fcode.p;
  if (h->st.stop_on) {
    L.stop_tail = b.stop_tail.p;
    L.stop_steps = b.stop_steps.p - first;
    L.stop_hit = b.stop_hit.p - first;
  }
  if (h->st.path_on && path) {
    L.path_D = b.path_D.p;
    L.path_p = b.path_p.p - first;
  } else {
    L.path_on = 0;
    L.path_D = L.path_p = nullptr;
  }
}

// The one-sample stage of sfw_score_one / sfw_score_one_crowd.  The agent set is checked before the stage (a refused call leaves
// the staged grid alone); past the checks the call consumes its stage, whatever the outcome (no grid to launch or dump)
int stage_one(sfw_handle h, const sfw_robot_state *rs, const sfw_goal_args *args, double vx, double vy, double vtheta) {
  const agent_set &ag = h->world.agents;
  if (int e = check_lds(h, ag.A, ag.O, ag.NG, ag.n_grp_mem, 1)) return e;
  return stage_common(h, rs, args, one_request(&vx, vy, &vtheta));
}
struct consume_stage {
  sfw_handle h;
  ~consume_stage() { h->st.valid = false; }
};

// sfw_score_one's outputs, wherever its kernels write them: cost (8) | n_points (4) | coll_step (4) | points (24 S)
constexpr size_t kOneHead = 16;
void score_one_outputs_at(sfw_launch &L, char *base) {
  L.costs = reinterpret_cast<double *>(base);
  L.n_points = reinterpret_cast<int32_t *>(base + 8);
  L.coll_step = reinterpret_cast<int32_t *>(base + 12);
  L.points = reinterpret_cast<double *>(base + kOneHead);
}
// The points of a Trajectory of n poses whose pedestrian contact step is coll (-1: none): rejected by contact at step c, the
// poses (steps) 0..c were added — addPoint precedes the test (ref :578, :613-627)
int32_t contact_trim(int32_t n, int32_t coll) { return (coll >= 0 && coll + 1 < n) ? coll + 1 : n; }
// ... and from a host copy of them to the caller
int32_t one_head_unpack(const char *src, double *cost_out) {  // -> the point (step) count
  int32_t n = 0, coll = -1;
  if (cost_out) std::memcpy(cost_out, src, sizeof(double));
  std::memcpy(&n, src + 8, sizeof(n));
  std::memcpy(&coll, src + 12, sizeof(coll));
  return contact_trim(n, coll);
}
void score_one_unpack(const char *src, double *cost_out, double *points_xyth, int32_t points_cap, int32_t *n_points) {
  const int32_t n = one_head_unpack(src, cost_out);
  if (n_points) *n_points = n;
  if (points_xyth && points_cap > 0 && n > 0) {
    const int m = n < points_cap ? n : points_cap;
    std::memcpy(points_xyth, src + kOneHead, sizeof(double) * 3 * static_cast<size_t>(m));
  }
}

// Samples [first, first + count) with count >= 1 inside [0, n)
bool sample_range_ok(int64_t first, int64_t count, int64_t n) { return first >= 0 && count >= 1 && first < n && count <= n - first; }
}  // namespace

extern "C" {

void sfw_params_default(sfw_params *p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  // ControllerParams defaults, reference sfw_planner.hpp:56-66
  p->max_vel_x = 0.7;
  p->sim_time = 1.0;
  p->sim_granularity = 0.025;
  p->robot_radius = 0.35f;
  p->social_weight = 1.2;
  p->costmap_weight = 2.0;
  p->angle_weight = 0.7;
  p->distance_weight = 1.0;
  p->vel_weight = 1.0;
  p->robot_goal_radius = 0.20;  // reference src/sfw_planner.cpp:608
  // lightsfm sfm::Parameters defaults
  p->sfm_force_factor_desired = 2.0;
  p->sfm_force_factor_obstacle = 10.0;
  p->sfm_force_sigma_obstacle = 0.2;
  p->sfm_force_factor_social = 2.1;
  p->sfm_lambda = 2.0;
  p->sfm_gamma = 0.35;
  p->sfm_n = 2.0;
  p->sfm_n_prime = 3.0;
  p->sfm_relaxation_time = 0.5;
  p->sfm_force_factor_group_gaze = 3.0;
  p->sfm_force_factor_group_coherence = 2.0;
  p->sfm_force_factor_group_repulsion = 1.0;
  p->precision = SFW_PRECISION_F64;
}

int sfw_abi_version(void) { return SFW_ABI_VERSION; }

}  // extern "C"

namespace {
int destroy_handle(sfw_handle h);
// A handle on its own streams (sfw_create), or on a batch's (stream / side non-null: borrowed, not destroyed with it)
int create_handle(const sfw_params *params, int device, hipStream_t stream, hipStream_t side, sfw_handle *out) {
  if (!out) return SFW_ERR_INVALID_ARG;
  *out = nullptr;
  if (int e = check_params(nullptr, params)) return e;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return SFW_ERR_NO_DEVICE;
  if (device < 0 || device >= count) return SFW_ERR_INVALID_ARG;
  sfw_handle h = new (std::nothrow) sfw_planner_s();
  if (!h) return SFW_ERR_HIP;
  h->live.params = *params;
  h->device = device;
  if (const char *b = std::getenv("SFW_PREFIX")) {  // "0" off, "10" one split, "3,7,12" several levels
    for (const char *q = b; *q;) {
      char *end = nullptr;
      const long v = std::strtol(q, &end, 10);
      if (end == q) break;
      if (v >= 0) h->cfg.prefix_env.push_back(static_cast<int>(v));
      q = (*end == ',') ? end + 1 : end;
    }
    std::sort(h->cfg.prefix_env.begin(), h->cfg.prefix_env.end());
    h->cfg.prefix_env.erase(std::unique(h->cfg.prefix_env.begin(), h->cfg.prefix_env.end()), h->cfg.prefix_env.end());
  }
  if (const char *b = std::getenv("SFW_FORCE_FLAT")) h->live.k2_form = std::atoi(b) == 1 ? SFW_K2_FLAT : std::atoi(b) == 0 ? SFW_K2_REGISTER : SFW_K2_AUTO;
  if (const char *b = std::getenv("SFW_PIN_REST")) h->cfg.pin_rest_on = std::atoi(b) != 0;
  if (const char *b = std::getenv("SFW_SPIN_US")) h->cfg.spin_us = std::max(0L, std::atol(b));
  if (const char *b = std::getenv("SFW_ARENA_DIRECT")) h->cfg.arena_direct_on = std::atoi(b) != 0;
  if (const char *b = std::getenv("SFW_MIRROR_MAX_MB")) h->cfg.mirror_max_bytes = static_cast<size_t>(std::max(0L, std::atol(b))) << 20;
  if (const char *b = std::getenv("SFW_OBS_TASKS")) h->cfg.obs_tasks_force = std::atoi(b) != 0 ? 1 : 0;
  if (const char *b = std::getenv("SFW_CLEAR_MIN_POSES")) h->cfg.clear_min_poses = std::max(0LL, std::atoll(b));
  if (const char *b = std::getenv("SFW_STOP_TABLE_ROWS")) h->cfg.stop_rows_max = std::max(0, std::atoi(b));
  if (const char *b = std::getenv("SFW_PATH_SLICES")) h->cfg.path_slices_on = std::atoi(b) != 0;
  if (const char *b = std::getenv("SFW_TABLE_BUDGET_MB")) {
    long mb = std::atol(b);
    if (mb > 0) h->cfg.table_budget_bytes = static_cast<size_t>(mb) << 20;
  }
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) {
    // the launch heuristics (shared-prefix cost model, organisation thresholds, XCD-contiguous block order) scale with the
    // device: a CPX partition of an MI355X shows 32 compute units on one XCD where the whole chip shows 256 on eight
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) h->cfg.n_cu = prop.multiProcessorCount;
    h->cfg.n_cu = env_device_cus(h->cfg.n_cu);
    // XCDs: what the device says (hipDeviceAttributeNumberOfXccs; 8 on a whole MI355X, 1 on a CPX partition) unless the CU count
    // is pretended (SFW_DEVICE_CUS) or the attribute is not answered — then CUs / 32, right for gfx950's 32-CU XCDs only
    int xccs = 0;
    if (!std::getenv("SFW_DEVICE_CUS") && hipDeviceGetAttribute(&xccs, hipDeviceAttributeNumberOfXccs, device) == hipSuccess && xccs >= 1)
      h->cfg.n_xcd = xccs;
    else
      h->cfg.n_xcd = std::max(1, h->cfg.n_cu / SFW_CUS_PER_XCD);
    (void)hipGetLastError();  // (an unanswered attribute is not an error of this call)
    if (const char *b = std::getenv("SFW_DEVICE_XCDS")) {
      const long v = std::atol(b);
      if (v >= 1 && v <= 64) h->cfg.n_xcd = static_cast<int>(v);
    }
  }
  if (stream) {
    h->cfg.owns_streams = false;
    h->stream = stream;
    h->side = side;
  } else {
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking);
  }
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_poses, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_side, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->split.fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->split.join, hipEventDisableTiming);
  if (e == hipSuccess) h->split.side = h->side;
  for (int i = 0; i < 5 && e == hipSuccess; ++i) e = hipEventCreate(&h->ev[i]);
  if (e == hipSuccess) e = h->cycle_counter.reserve(1);
  if (e == hipSuccess) e = hipMemsetAsync(h->cycle_counter.p, 0, sizeof(unsigned), h->stream);
  if (e != hipSuccess) {
    destroy_handle(h);
    return SFW_ERR_HIP;
  }
  *out = h;
  return SFW_OK;
}

int destroy_handle(sfw_handle h) {
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->side) (void)hipStreamSynchronize(h->side);
  h->cells.release();
  h->arena.release();
  h->pair_tab.release();
  h->crowd_pair_tab.release();
  h->crowd_out.release();
  h->pin_crowd.release();
  h->status.release();
  h->coll_step.release();
  h->base_cost.release();
  h->costs.release();
  h->ptab.release();
  h->cs_tab.release();
  h->fcode.release();
  h->clear_map.release();
  h->clear_tmp.release();
  h->partials.release();
  h->clock.release();
  h->cycle_counter.release();
  h->pin_cap.release();
  h->terms.release();
  h->rescore_w.release();
  h->rescore_partials.release();
  h->rescore_costs.release();
  h->pin_rescore.release();
  h->blend.release();
  h->mppi.release();
  h->normals.release();
  h->pin_knots.release();
  h->points.release();
  h->n_points.release();
  h->one_out.release();
  h->pts.release();
  h->stop_steps.release();
  h->stop_hit.release();
  h->stop_tail.release();
  h->stop_pts.release();
  h->path_seg.release();
  h->pin_path.release();
  h->path_D.release();
  h->path_p.release();
  h->rescore_pw.release();
  h->pin_map.release();
  h->pin_arena.release();
  h->pin_out.release();
  h->pin_mirror.release();
  h->pin_one.release();
  h->pin_cls.release();
  h->d_cls.release();
  for (auto &b : h->cls_dead) b.release();
  for (auto &b : h->cls_state) b.release();
  for (auto &e : h->ev)
    if (e) (void)hipEventDestroy(e);
  for (auto &e : h->chunk_ev)
    if (e) (void)hipEventDestroy(e);
  if (h->ev_poses) (void)hipEventDestroy(h->ev_poses);
  if (h->ev_side) (void)hipEventDestroy(h->ev_side);
  if (h->split.fork) (void)hipEventDestroy(h->split.fork);
  if (h->split.join) (void)hipEventDestroy(h->split.join);
  if (h->cfg.owns_streams) {
    if (h->side) (void)hipStreamDestroy(h->side);
    if (h->stream) (void)hipStreamDestroy(h->stream);
  }
  delete h;
  return SFW_OK;
}
}  // namespace

extern "C" {

int sfw_create(const sfw_params *params, int device, sfw_handle *out) {
  return create_handle(params, device, nullptr, nullptr, out);
}

int sfw_destroy(sfw_handle h) {
  if (!h) return SFW_OK;
  if (h->cfg.batch_member) return fail(h, SFW_ERR_STATE, "destroy: the handle is a member of a batch (sfw_batch_destroy destroys it)");
  return destroy_handle(h);
}

int sfw_set_params(sfw_handle h, const sfw_params *params) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (int e = check_params(h, params)) return e;
  if (std::memcmp(&h->live.params, params, sizeof(sfw_params)) != 0) ++h->live.params_epoch;
  h->live.params = *params;
  return SFW_OK;
}

const char *sfw_last_error(sfw_handle h) { return h ? h->err.c_str() : "null handle"; }

int sfw_set_costmap(sfw_handle h, const uint8_t *cells, uint32_t size_x, uint32_t size_y, double origin_x,
                    double origin_y, double resolution) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!cells || size_x == 0 || size_y == 0 || !(resolution > 0))
    return fail(h, SFW_ERR_INVALID_ARG, "set_costmap: null cells, zero size or non-positive resolution");
  // A NaN origin passes every `wx < origin` rejection and lands every pose in cell (0, 0); an infinite resolution or origin
  // does the like.  The two size limits are what the kernels' cell arithmetic is good for (sfw_hip.h; sfw_kernels.hip cell_index).
  if (!std::isfinite(origin_x) || !std::isfinite(origin_y) || !std::isfinite(resolution))
    return fail(h, SFW_ERR_INVALID_ARG, "set_costmap: origin or resolution is not finite");
  if (size_x > SFW_MAX_MAP_AXIS_CELLS || size_y > SFW_MAX_MAP_AXIS_CELLS || static_cast<uint64_t>(size_x) * size_y > SFW_MAX_MAP_CELLS)
    return fail(h, SFW_ERR_INVALID_ARG, "set_costmap: more than SFW_MAX_MAP_AXIS_CELLS cells on an axis or SFW_MAX_MAP_CELLS in all");
  SFW_HIP(h, hipSetDevice(h->device));
  const size_t n = static_cast<size_t>(size_x) * size_y;
  // The snapshot is taken here (the caller's buffer may change on return) and reaches the device with the NEXT stage — like
  // footprint and agents — as part of that stage's one arena copy when it is small (a control cycle's local costmap: one
  // copy per cycle instead of two with the host's call-to-call latency between them), by a copy of its own otherwise.
  // (an unchanged snapshot — a controller hands its local costmap over every cycle, the map changes at the costmap's own
  // rate — is recognised here, ~1 us for 40 KB, and not sent again)
  if (h->world.have_costmap && h->pin_map.p && n <= h->pin_map.cap && h->world.map_new.size_x == size_x && h->world.map_new.size_y == size_y &&
      h->world.map_new.origin_x == origin_x && h->world.map_new.origin_y == origin_y && h->world.map_new.resolution == resolution &&
      std::memcmp(h->pin_map.p, cells, n) == 0)
    return SFW_OK;
  SFW_HIP(h, h->pin_map.reserve(n));  // (waits for a copy out of it that is still pending)
  std::memcpy(h->pin_map.p, cells, n);
  h->world.map_new = {size_x, size_y, origin_x, origin_y, resolution};
  h->world.cells_dirty = true;
  ++h->world.cells_gen;
  h->world.have_costmap = true;
  return SFW_OK;
}

int sfw_set_footprint(sfw_handle h, const double *xy, int32_t K) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (K < 0 || (K > 0 && !xy)) return fail(h, SFW_ERR_INVALID_ARG, "set_footprint: bad arguments");
  h->world.footprint.assign(xy, xy + 2 * static_cast<size_t>(K));  // uploaded with the next stage
  h->world.K = K;
  return SFW_OK;
}

int sfw_set_agents(sfw_handle h, const sfw_agent *agents, int32_t A, const double *obstacles_xy, int32_t O) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (A < 0 || O < 0 || (A > 0 && !agents) || (O > 0 && !obstacles_xy))
    return fail(h, SFW_ERR_INVALID_ARG, "set_agents: bad arguments");
  for (int i = 0; i < A; ++i) {
    const sfw_agent &a = agents[i];
    if (!all_finite(&a.x, 4) || !std::isfinite(a.desired_velocity) || !std::isfinite(a.radius) ||
        (a.has_goal && !(all_finite(&a.goal_x, 2) && std::isfinite(a.goal_radius))))
      return fail(h, SFW_ERR_INVALID_ARG, "set_agents: non-finite field in agent " + std::to_string(i));
    // desired_velocity <= 0 is accepted, as the reference accepts people_velocity_ = 0 (sensor_interface.cpp:503): the speed
    // clamp of lightsfm's updatePosition pins such a person where it stands (include/sfw_hip.h, sfw_agent)
  }
  if (O > 0 && !all_finite(obstacles_xy, 2 * static_cast<size_t>(O)))
    return fail(h, SFW_ERR_INVALID_ARG, "set_agents: non-finite laser point");
  // The flat K2 addresses an agent's LDS words through 16-bit byte offsets (pair table) and the whole set has to fit one
  // wave's LDS allocation long before that: refused here, not as a failed launch later
  if (A > 8190) return fail(h, SFW_ERR_UNSUPPORTED, "set_agents: more than 8190 agents");
  const size_t An = static_cast<size_t>(A > 0 ? A : 1), On = static_cast<size_t>(O > 0 ? O : 1);
  // groups: dense index in order of first appearance, CSR member lists in agent order
  std::vector<int32_t> grp(An, -1), ids, off(1, 0), mem;
  for (int i = 0; i < A; ++i) {
    if (agents[i].group_id < 0) continue;
    size_t q = 0;
    while (q < ids.size() && ids[q] != agents[i].group_id) ++q;
    if (q == ids.size()) ids.push_back(agents[i].group_id);
    grp[i] = static_cast<int32_t>(q);
  }
  for (size_t q = 0; q < ids.size(); ++q) {
    for (int i = 0; i < A; ++i)
      if (grp[i] == static_cast<int32_t>(q)) mem.push_back(i);
    off.push_back(static_cast<int32_t>(mem.size()));
  }
  const int n_mem = off.back();
  // the set has to fit one wave's LDS allocation whatever the grid (the flat form of one sample is the smallest): refused
  // here, before the all-pairs scan below and long before a launch
  if (A > 0 && sfw_social_lds_bytes(A, O, static_cast<int>(ids.size()), n_mem, 1, SFW_K2_FLAT, h->cfg.n_cu) > 160 * 1024)
    return fail(h, SFW_ERR_UNSUPPORTED, "set_agents: agent/obstacle set does not fit the 160 KiB LDS of one CU");
  if (mem.empty()) mem.push_back(0);
  // host blob (uploaded with the next stage): pos | vel | const | obstacles | grp | off | mem
  auto up16 = [](size_t b) { return (b + 15) & ~size_t(15); };
  const size_t o_pos = 0, o_vel = o_pos + up16(16 * An), o_cst = o_vel + up16(16 * An),
               o_obs = o_cst + up16(sizeof(sfw_agent_const) * An),
               // + 64 behind the points: the kernels read them in groups of four (s_load_dwordx16) and, in the flat form's task
               // loop, up to two points ahead of the one being evaluated, without clamping the index (loaded, never used)
               o_grp = o_obs + up16(16 * On) + 64,
               o_off = o_grp + up16(4 * An), o_mem = o_off + up16(4 * off.size()),
               total = o_mem + up16(4 * mem.size());
  agent_set &ag = h->world.agents;
  ag.blob.assign(total, 0);
  char *base = ag.blob.data();
  double *pos = reinterpret_cast<double *>(base + o_pos), *vel = reinterpret_cast<double *>(base + o_vel);
  sfw_agent_const *cst = reinterpret_cast<sfw_agent_const *>(base + o_cst);
  ag.person_pinned = false;
  for (int i = 0; i < A; ++i) {
    pos[2 * i] = agents[i].x;
    pos[2 * i + 1] = agents[i].y;
    vel[2 * i] = agents[i].vx;
    vel[2 * i + 1] = agents[i].vy;
    sfw_agent_const &c = cst[i];
    c.goal_x = agents[i].goal_x;
    c.goal_y = agents[i].goal_y;
    c.goal_radius = agents[i].goal_radius;
    c.desired_velocity = agents[i].desired_velocity;
    c.radius = agents[i].radius;
    c.id = agents[i].id;
    c.has_goal = agents[i].has_goal ? 1 : 0;
    ag.person_pinned |= i >= 1 && c.desired_velocity == 0.0;
  }
  if (O > 0) std::memcpy(base + o_obs, obstacles_xy, sizeof(double) * 2 * O);
  std::memcpy(base + o_grp, grp.data(), 4 * grp.size());
  std::memcpy(base + o_off, off.data(), 4 * off.size());
  std::memcpy(base + o_mem, mem.data(), 4 * mem.size());
  ag.ao_vel = o_vel;
  ag.ao_cst = o_cst;
  ag.ao_obs = o_obs;
  ag.ao_grp = o_grp;
  ag.ao_off = o_off;
  ag.ao_mem = o_mem;
  ag.NG = static_cast<int>(ids.size());
  ag.n_grp_mem = n_mem;
  ag.A = A;
  ag.O = O;
  // Pairs whose w x diff is exactly 0 in the handed-over state — relative rest (w = 0) and motion exactly along the
  // connecting line — are the pairs for which the kernels' sign(theta) = sign(w x diff) is 0 while lightsfm's theta is
  // rounding noise around 0 or exactly +-pi: their angular terms are evaluated on the host (rest_forces).  The test is
  // the kernels' own expression (pair_force_state), IEEE fma on both sides.  All pairs: ~1 ns each, 1275 at 50
  // pedestrians; the scoring that follows costs A^2 per sample-step.
  ag.rest_pairs.clear();
  for (int i = 0; i < A; ++i)
    for (int j = i + 1; j < A; ++j) {
      const double dx = agents[j].x - agents[i].x, dy = agents[j].y - agents[i].y;
      const double wx = agents[i].vx - agents[j].vx, wy = agents[i].vy - agents[j].vy;
      if (std::fma(wx, dy, -(wy * dx)) == 0.0 && !(dx == 0.0 && dy == 0.0)) {
        ag.rest_pairs.emplace_back(i, j);
        ag.rest_pairs.emplace_back(j, i);
      }
    }
  return SFW_OK;
}

int sfw_grid_stage(sfw_handle h, const sfw_robot_state *rs, const double *linvels, int32_t nv,
                   const double *angvels, int32_t nw, const sfw_goal_args *args, int64_t index_base) {
  return stage_common(h, rs, args, grid_request(linvels, nv, angvels, nw, index_base));
}

int sfw_samples_stage(sfw_handle h, const sfw_robot_state *rs, const double *vx, const double *vy, const double *vtheta,
                      int32_t n, const sfw_goal_args *args, int64_t index_base) {
  return stage_common(h, rs, args, list_request(vx, vy, vtheta, n, index_base));
}

int sfw_sequences_stage(sfw_handle h, const sfw_robot_state *rs, const double *vx, const double *vy, const double *vtheta,
                        int32_t n, int32_t K, const int32_t *knot_step, const sfw_goal_args *args, int64_t index_base) {
  if (!h) return SFW_ERR_INVALID_ARG;
  // (refused before anything is touched: the staged grid, list or sequences stay launchable)
  if (const char *why = sequences_refusal(K, knot_step)) return fail(h, SFW_ERR_INVALID_ARG, std::string("sequences_stage: ") + why);
  return stage_common(h, rs, args, sequences_request(vx, vy, vtheta, n, K, knot_step, index_base));
}

int sfw_grid_launch(sfw_handle h) { return launch_common(h); }

int sfw_grid_sync(sfw_handle h) {
  if (!h) return SFW_ERR_INVALID_ARG;
  SFW_HIP(h, hipSetDevice(h->device));
  SFW_HIP(h, hipStreamSynchronize(h->stream));
  return SFW_OK;
}

int sfw_grid_fetch(sfw_handle h, double *costs_out, sfw_best *best_out, sfw_best_key *key_out) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!h->last.launched) return fail(h, SFW_ERR_STATE, "grid_fetch before grid_launch");
  SFW_HIP(h, hipSetDevice(h->device));
  const int64_t T = static_cast<int64_t>(h->st.nv) * h->st.nw;
  // costs and the selection record are contiguous on the device: one copy fetches both
  sfw_sel s;
  if (h->last.mirrored) {  // the launch's selection kernels wrote both to pin_mirror: nothing to copy, only to wait for
    const size_t all_bytes = sizeof(double) * static_cast<size_t>(T);
    SFW_HIP(h, wait_stream(h));
    h->last.fetched = true;
    if (costs_out) std::memcpy(costs_out, h->pin_mirror.p, all_bytes);
    std::memcpy(&s, h->pin_mirror.p + all_bytes, sizeof(s));
  } else {
    const size_t cost_bytes = costs_out ? sizeof(double) * static_cast<size_t>(T) : 0;
    SFW_HIP(h, h->pin_out.reserve(cost_bytes + sizeof(sfw_sel)));
    const char *src = reinterpret_cast<const char *>(h->st.d_sel) - cost_bytes;
    SFW_HIP(h, hipMemcpyAsync(h->pin_out.p, src, cost_bytes + sizeof(sfw_sel), hipMemcpyDeviceToHost, h->stream));
    SFW_HIP(h, wait_stream(h));
    h->last.fetched = true;
    if (costs_out) std::memcpy(costs_out, h->pin_out.p, cost_bytes);
    std::memcpy(&s, h->pin_out.p + cost_bytes, sizeof(s));
  }
  return sel_to_best(h, s, best_out, key_out);
}

const double *sfw_grid_costs_view(sfw_handle h) {
  if (!h || !h->last.launched || !h->last.mirrored || !h->last.fetched) return nullptr;
  return reinterpret_cast<const double *>(h->pin_mirror.p);
}

int sfw_score_grid(sfw_handle h, const sfw_robot_state *rs, const double *linvels, int32_t nv,
                   const double *angvels, int32_t nw, const sfw_goal_args *args, double *costs_out,
                   sfw_best *best_out) {
  return score_staged(h, sfw_grid_stage(h, rs, linvels, nv, angvels, nw, args, 0), costs_out, best_out);
}

int sfw_score_samples(sfw_handle h, const sfw_robot_state *rs, const double *vx, const double *vy, const double *vtheta,
                      int32_t n, const sfw_goal_args *args, double *costs_out, sfw_best *best_out) {
  return score_staged(h, sfw_samples_stage(h, rs, vx, vy, vtheta, n, args, 0), costs_out, best_out);
}

int sfw_score_sequences(sfw_handle h, const sfw_robot_state *rs, const double *vx, const double *vy, const double *vtheta,
                        int32_t n, int32_t K, const int32_t *knot_step, const sfw_goal_args *args, double *costs_out,
                        sfw_best *best_out) {
  return score_staged(h, sfw_sequences_stage(h, rs, vx, vy, vtheta, n, K, knot_step, args, 0), costs_out, best_out);
}

int sfw_sequences_perturb_stage(sfw_handle h, const sfw_robot_state *rs, const sfw_perturb *p, int32_t n, int32_t K,
                                const int32_t *knot_step, const sfw_goal_args *args, int64_t index_base) {
  if (!h) return SFW_ERR_INVALID_ARG;
  // (refused before anything is touched: the staged grid, list or sequences stay launchable)
  if (const char *why = perturb_refusal(rs, p, n, K, knot_step, args, index_base))
    return fail(h, SFW_ERR_INVALID_ARG, std::string("sequences_perturb_stage: ") + why);
  const bool no_vy = (p->flags & SFW_PERTURB_NO_VY) != 0;
  perturb_source src{};
  perturb_seed(src.args, p->seed);
  src.args.keep_nominal = (p->flags & SFW_PERTURB_KEEP_NOMINAL) ? 1 : 0;
  for (int c = 0; c < 3; ++c) {
    src.args.sigma[c] = p->sigma[c];
    src.args.lo[c] = p->lo[c];
    src.args.hi[c] = p->hi[c];
  }
  std::memcpy(src.args.nominal, p->nominal, sizeof(double) * 3 * static_cast<size_t>(K));
  src.vy = !no_vy;
  src.keep_normals = (p->flags & SFW_PERTURB_KEEP_NORMALS) != 0;
  src.zero_admitted = p->lo[0] <= 0.0 && 0.0 <= p->hi[0] && (no_vy || (p->lo[1] <= 0.0 && 0.0 <= p->hi[1]));
  return stage_common(h, rs, args, perturbed_request(&src, n, K, knot_step, index_base));
}

int sfw_score_perturbed(sfw_handle h, const sfw_robot_state *rs, const sfw_perturb *p, int32_t n, int32_t K,
                        const int32_t *knot_step, const sfw_goal_args *args, double *costs_out, sfw_best *best_out) {
  return score_staged(h, sfw_sequences_perturb_stage(h, rs, p, n, K, knot_step, args, 0), costs_out, best_out);
}

int sfw_sequences_knots(sfw_handle h, int64_t first, int64_t count, double *vx_out, double *vy_out, double *vtheta_out) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!h->st.valid || !h->st.list) return fail(h, SFW_ERR_STATE, "sequences_knots: no list or sequences are staged");
  const int64_t n = h->st.nv;
  if (!sample_range_ok(first, count, n)) return fail(h, SFW_ERR_INVALID_ARG, "sequences_knots: range outside [0, n)");
  if (!vx_out || !vtheta_out) return fail(h, SFW_ERR_INVALID_ARG, "sequences_knots: vx_out or vtheta_out is NULL");
  const size_t K = static_cast<size_t>(h->st.nk), cnt = static_cast<size_t>(count);
  double *const out[3] = {vx_out, vy_out, vtheta_out};
  if (h->st.perturbed) {
    const double *rows[3];
    if (int e = knots_from_device(h, first, count, rows)) return e;
    for (int c = 0; c < 3; ++c) {
      if (!out[c]) continue;
      if (rows[c]) std::memcpy(out[c], rows[c], sizeof(double) * K * cnt);
      else std::fill(out[c], out[c] + K * cnt, 0.0);
    }
    return SFW_OK;
  }
  // a host-staged list or sequences: the stage's own record of what it uploaded
  const std::vector<double> *const src[3] = {&h->st.lin, h->st.vy.empty() ? nullptr : &h->st.vy, &h->st.ang};
  for (int c = 0; c < 3; ++c) {
    if (!out[c]) continue;
    for (size_t k = 0; k < K; ++k) {
      if (src[c]) std::memcpy(out[c] + k * cnt, src[c]->data() + k * static_cast<size_t>(n) + first, sizeof(double) * cnt);
      else std::fill(out[c] + k * cnt, out[c] + (k + 1) * cnt, 0.0);
    }
  }
  return SFW_OK;
}

int sfw_sequences_normals(sfw_handle h, int64_t first, int64_t count, double *z_out) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!h->st.valid || !h->st.perturbed || !h->st.normals_kept)
    return fail(h, SFW_ERR_STATE, "sequences_normals: no perturbed stage with SFW_PERTURB_KEEP_NORMALS is staged");
  const int64_t n = h->st.nv;
  if (!sample_range_ok(first, count, n)) return fail(h, SFW_ERR_INVALID_ARG, "sequences_normals: range outside [0, n)");
  if (!z_out) return fail(h, SFW_ERR_INVALID_ARG, "sequences_normals: z_out is NULL");
  const size_t rows = 3 * static_cast<size_t>(h->st.nk), row = sizeof(double) * static_cast<size_t>(count);
  SFW_HIP(h, hipSetDevice(h->device));
  if (rows * row > h->pin_knots.cap) SFW_HIP(h, hipStreamSynchronize(h->stream));  // (growing the area frees the old one)
  SFW_HIP(h, h->pin_knots.reserve(rows * row));
  SFW_HIP(h, hipMemcpy2DAsync(h->pin_knots.p, row, h->normals.p + first, sizeof(double) * static_cast<size_t>(n), row, rows,
                              hipMemcpyDeviceToHost, h->stream));
  SFW_HIP(h, wait_stream(h));
  std::memcpy(z_out, h->pin_knots.p, rows * row);
  return SFW_OK;
}

int sfw_score_one(sfw_handle h, const sfw_robot_state *rs, double vx_samp, double vy_samp, double vtheta_samp,
                  const sfw_goal_args *args, double *cost_out, double *points_xyth, int32_t points_cap,
                  int32_t *n_points) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!cost_out) return fail(h, SFW_ERR_INVALID_ARG, "score_one: cost_out is NULL");
  if (int e = stage_one(h, rs, args, vx_samp, vy_samp, vtheta_samp)) return e;
  consume_stage consumed{h};
  const int S = num_steps_of(h->live.params);
  // cost (8) | n_points (4) | coll_step (4) | points (24 S), contiguous
  const size_t head = kOneHead, pts_bytes = sizeof(double) * 3 * static_cast<size_t>(S);
  sfw_launch L;
  fill_launch(h, L, 0, 1, 1);
  // With points wanted a costmap-rejected sample is integrated too: a pedestrian contact at an earlier step ends the
  // reference's Trajectory there (ref :613-627 returns before the later illegal pose is ever reached)
  L.force_alive = (points_xyth && points_cap > 0) || n_points ? 1 : 0;
  {
    // The latency path (called on every approach / rotate cycle, ref :204-206, :299-301) as ONE launch and no copy: the
    // one-launch kernel with its outputs — cost, point count, contact step, Trajectory points — in pinned host memory, the
    // stage's arena fetched by the kernel (stage_common left it pending), no selection.
    sfw_launch C = L;
    C.sel_out = nullptr;
    C.cycle_counter = nullptr;
    if (sfw_cycle_applies(C)) {
      if (head + pts_bytes > h->pin_one.cap) SFW_HIP(h, hipStreamSynchronize(h->stream));  // (growing it frees the old area)
      SFW_HIP(h, h->pin_one.reserve(head + pts_bytes));
      score_one_outputs_at(C, h->pin_one.p);
      arena_by_kernel(h, C);
      SFW_HIP(h, launch_cycle_of(C, h->stream));
      SFW_HIP(h, arena_fetched(h));
      SFW_HIP(h, wait_stream(h));
      score_one_unpack(h->pin_one.p, cost_out, points_xyth, points_cap, n_points);
      return SFW_OK;
    }
    if (int e = flush_arena(h)) return e;  // the three-kernel path below reads the device copy
  }
  // ... else on the device, so that the call pays one pinned D2H, like sfw_grid_fetch
  SFW_HIP(h, h->one_out.reserve(head + pts_bytes));
  score_one_outputs_at(L, h->one_out.p);
  SFW_HIP(h, sfw_launch_rollout(L, h->stream));
  SFW_HIP(h, launch_social_of(L, h->stream));
  if (L.path_on) SFW_HIP(h, sfw_launch_path_add(L.costs, L.path_p, h->st.path_weight, 0, 1, h->stream));
  const size_t fetch = head + ((points_xyth && points_cap > 0) ? pts_bytes : 0);
  SFW_HIP(h, h->pin_out.reserve(fetch));
  SFW_HIP(h, hipMemcpyAsync(h->pin_out.p, h->one_out.p, fetch, hipMemcpyDeviceToHost, h->stream));
  SFW_HIP(h, hipStreamSynchronize(h->stream));
  score_one_unpack(h->pin_out.p, cost_out, points_xyth, points_cap, n_points);
  return SFW_OK;
}

// sfw_plan_shared_prefix (items false: the velocity classes of each level) and sfw_plan_shared_prefix_items (items true: its
// work items, whose column axis lags by one step) of ONE plan
static int plan_shared_prefix(const double *linvels, int32_t nv, const double *angvels, int32_t nw, double vx0, double vtheta0,
                              double acc_x, double acc_theta, double sim_time, int32_t num_steps, int32_t n_agents,
                              int32_t *level_ends, int64_t *level_classes, int32_t cap, int32_t *n_levels, bool items) {
  if (!linvels || !angvels || nv <= 0 || nw <= 0 || num_steps < 1 || !n_levels || cap < 0 ||
      (cap > 0 && (!level_ends || !level_classes)))
    return SFW_ERR_INVALID_ARG;
  *n_levels = 0;
  const int64_t T = static_cast<int64_t>(nv) * nw;
  if (n_agents < 2 || num_steps < 2 || T < 4096) return SFW_OK;
  const std::vector<double> lin(linvels, linvels + nv), ang(angvels, angvels + nw);
  prefix_classes pc;
  classes_of_grid(pc, lin, ang, vx0, vtheta0, acc_x, acc_theta, sim_time / num_steps, num_steps);
  const int cus = env_device_cus(SFW_DEFAULT_CUS);  // host only: no device to ask
  const std::vector<int> steps = choose_levels(pc, T, num_steps, static_cast<double>(sfw_samples_per_wave(n_agents, T, SFW_K2_AUTO, cus)), cus);
  *n_levels = static_cast<int32_t>(steps.size());
  for (size_t l = 0; l < steps.size() && l < static_cast<size_t>(cap); ++l) {
    level_ends[l] = steps[l];
    level_classes[l] = items ? pc.n_items_at(steps[l]) : static_cast<int64_t>(pc.n_rows_at(steps[l])) * pc.n_cols_at(steps[l]);
  }
  return SFW_OK;
}
int sfw_plan_shared_prefix(const double *linvels, int32_t nv, const double *angvels, int32_t nw, double vx0, double vtheta0,
                           double acc_x, double acc_theta, double sim_time, int32_t num_steps, int32_t n_agents,
                           int32_t *level_ends, int64_t *level_classes, int32_t cap, int32_t *n_levels) {
  return plan_shared_prefix(linvels, nv, angvels, nw, vx0, vtheta0, acc_x, acc_theta, sim_time, num_steps, n_agents, level_ends,
                            level_classes, cap, n_levels, false);
}
int sfw_plan_shared_prefix_items(const double *linvels, int32_t nv, const double *angvels, int32_t nw, double vx0, double vtheta0,
                                 double acc_x, double acc_theta, double sim_time, int32_t num_steps, int32_t n_agents,
                                 int32_t *level_ends, int64_t *level_items, int32_t cap, int32_t *n_levels) {
  return plan_shared_prefix(linvels, nv, angvels, nw, vx0, vtheta0, acc_x, acc_theta, sim_time, num_steps, n_agents, level_ends,
                            level_items, cap, n_levels, true);
}

int sfw_plan_axis_classes(const double *targets, int32_t n, double v0, double a_max, double dt, int32_t max_p, int32_t form,
                          int32_t *counts, int32_t *classes, int32_t *n_levels, int32_t *closed_form) {
  if (!targets || n <= 0 || max_p < 1 || !counts || !n_levels || (form != 0 && form != 1)) return SFW_ERR_INVALID_ARG;
  if (!all_finite(targets, static_cast<size_t>(n)) || !std::isfinite(v0) || !std::isfinite(a_max) || !std::isfinite(dt))
    return SFW_ERR_INVALID_ARG;
  const axis_classes a = classes_of_axis(std::vector<double>(targets, targets + n), v0, a_max, dt, max_p, form == 0);
  *n_levels = static_cast<int32_t>(a.n.size());
  if (closed_form) *closed_form = a.fast ? 1 : 0;
  for (size_t l = 0; l < a.n.size(); ++l) {
    counts[l] = a.n[l];
    if (classes) std::memcpy(classes + l * static_cast<size_t>(n), a.level(static_cast<int>(l) + 1).data(), sizeof(int32_t) * static_cast<size_t>(n));
  }
  return SFW_OK;
}

int sfw_plan_row_blocks(const double *linvels, int32_t nv, const double *angvels, int32_t nw, double vx0, double vtheta0,
                        double acc_x, double acc_theta, double sim_time, int32_t num_steps, int32_t n_agents, int32_t R,
                        int32_t *row0) {
  if (!linvels || !angvels || nv <= 0 || nw <= 0 || num_steps < 1 || R < 1 || !row0) return SFW_ERR_INVALID_ARG;
  if (!all_finite(linvels, static_cast<size_t>(nv)) || !all_finite(angvels, static_cast<size_t>(nw))) return SFW_ERR_INVALID_ARG;
  const std::vector<double> lin(linvels, linvels + nv), ang(angvels, angvels + nw);
  std::vector<int32_t> cuts;
  plan_row_blocks(lin, ang, vx0, vtheta0, acc_x, acc_theta, sim_time / num_steps, num_steps, n_agents, R, SFW_K2_AUTO,
                  env_device_cus(SFW_DEFAULT_CUS), cuts);
  std::memcpy(row0, cuts.data(), sizeof(int32_t) * (static_cast<size_t>(R) + 1));
  return SFW_OK;
}

int sfw_grid_plan_info(sfw_handle h, sfw_plan_info *out) {
  if (!h || !out) return SFW_ERR_INVALID_ARG;
  if (!h->st.valid) return fail(h, SFW_ERR_STATE, "grid_plan_info before grid_stage");
  const int64_t T = static_cast<int64_t>(h->st.nv) * h->st.nw;
  out->split_step = h->st.prefix_steps.empty() ? 0 : h->st.prefix_steps.back();
  out->levels = static_cast<int32_t>(h->st.prefix_steps.size());
  out->samples = T;
  out->classes = h->st.prefix_last_classes;
  out->class_steps = h->st.prefix_class_steps;
  if (!h->st.prefix_steps.empty()) {
    out->chunks = static_cast<int32_t>(h->st.prefix_chunks.size());
  } else {
    int64_t chunk = h->st.table_chunk;
    if (chunk > T) chunk = T;
    out->chunks = chunk > 0 ? static_cast<int32_t>((T + chunk - 1) / chunk) : 0;
  }
  out->organisation = sfw_social_organisation(h->st.A, out->chunks > 0 ? (T + out->chunks - 1) / out->chunks : T, h->st.O, h->live.k2_form, h->cfg.n_cu);
  out->flat_samples = sfw_social_flat_items(h->st.A, h->st.O, h->st.NG, out->chunks > 0 ? (T + out->chunks - 1) / out->chunks : T, h->live.k2_form, h->cfg.n_cu);
  out->rest_noise_unreproduced = rest_noise_unreproduced(h) ? 1 : 0;
  out->one_launch = 0;
  if (out->chunks == 1 && h->st.prefix_steps.empty()) {
    sfw_launch L;
    fill_launch(h, L, 0, T, T);
    out->one_launch = sfw_cycle_applies(L) ? 1 : 0;
  }
  return SFW_OK;
}

int sfw_set_k2_form(sfw_handle h, int32_t form) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (form != SFW_K2_AUTO && form != SFW_K2_REGISTER && form != SFW_K2_FLAT)
    return fail(h, SFW_ERR_INVALID_ARG, "set_k2_form: form must be SFW_K2_AUTO, SFW_K2_REGISTER or SFW_K2_FLAT");
  h->live.k2_form = form;
  return SFW_OK;
}

int sfw_set_timing(sfw_handle h, int32_t enabled) {
  if (!h) return SFW_ERR_INVALID_ARG;
  h->live.timing = enabled != 0;
  return SFW_OK;
}

int sfw_last_launch_ms(sfw_handle h, int32_t which, float *ms_out) {
  if (!h || !ms_out) return SFW_ERR_INVALID_ARG;
  if (!h->last.launched) return fail(h, SFW_ERR_STATE, "last_launch_ms before grid_launch");
  if (!h->last.timed) return fail(h, SFW_ERR_STATE, "last_launch_ms: timing was off for the last launch (sfw_set_timing)");
  SFW_HIP(h, hipSetDevice(h->device));
  SFW_HIP(h, hipEventSynchronize(h->ev[3]));
  if (h->last.n_chunks > 1 && (which == 1 || which == 2)) {  // sum over the chunks of a multi-chunk launch
    float total = 0.0f;
    for (int c = 0; c < h->last.n_chunks; ++c) {
      float ms = 0.0f;
      const int a = 3 * c + (which == 1 ? 0 : 1);
      SFW_HIP(h, hipEventElapsedTime(&ms, h->chunk_ev[a], h->chunk_ev[a + 1]));
      total += ms;
    }
    *ms_out = total;
    return SFW_OK;
  }
  int a = 0, b = 3;
  switch (which) {
    case 0: a = 0; b = 3; break;
    case 1: a = 0; b = 1; break;
    case 2: a = 1; b = 2; break;
    case 3: a = 2; b = 3; break;
    default: return fail(h, SFW_ERR_INVALID_ARG, "last_launch_ms: which must be 0..3");
  }
  SFW_HIP(h, hipEventElapsedTime(ms_out, h->ev[a], h->ev[b]));
  return SFW_OK;
}

int sfw_set_points_capture(sfw_handle h, int32_t enabled) {
  if (!h) return SFW_ERR_INVALID_ARG;
  h->live.capture_points = enabled != 0;
  return SFW_OK;
}

int sfw_set_footprint_clearance(sfw_handle h, int32_t on) {
  if (!h) return SFW_ERR_INVALID_ARG;
  h->live.fp_clear = on != 0;
  return SFW_OK;
}

int sfw_footprint_clearance_info(sfw_handle h, int32_t *built, int32_t *half_width) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!built || !half_width) return fail(h, SFW_ERR_INVALID_ARG, "footprint_clearance_info: null pointer");
  if (!h->st.valid) return fail(h, SFW_ERR_STATE, "footprint_clearance_info: nothing is staged");
  *built = (h->live.fp_clear && h->st.clear_on) ? 1 : 0;
  *half_width = h->st.clear_r;
  return SFW_OK;
}

int sfw_footprint_clearance_map(sfw_handle h, uint8_t *out, uint64_t cells) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!h->st.valid || !h->st.clear_on) return fail(h, SFW_ERR_STATE, "footprint_clearance_map: the staged grid has no clearance map");
  if (!out || cells != static_cast<uint64_t>(h->st.map.size_x) * h->st.map.size_y)
    return fail(h, SFW_ERR_INVALID_ARG, "footprint_clearance_map: null buffer, or not size_x * size_y cells");
  SFW_HIP(h, hipSetDevice(h->device));
  SFW_HIP(h, hipMemcpyAsync(out, h->clear_map.p, cells, hipMemcpyDeviceToHost, h->stream));
  SFW_HIP(h, hipStreamSynchronize(h->stream));
  return SFW_OK;
}

int sfw_set_stop_check(sfw_handle h, const sfw_stop_check *c) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!c) {
    h->live.stop_on = false;
    h->live.stop = sfw_stop_check{};
    return SFW_OK;
  }
  for (double d : {c->dec_x, c->dec_y, c->dec_theta})
    if (!std::isfinite(d) || d < 0) return fail(h, SFW_ERR_INVALID_ARG, "set_stop_check: a braking limit is not finite or below 0");
  if (c->max_steps < 1 || c->max_steps > SFW_STOP_MAX_STEPS)
    return fail(h, SFW_ERR_INVALID_ARG, "set_stop_check: max_steps outside 1 .. SFW_STOP_MAX_STEPS");
  if (c->reserved != 0) return fail(h, SFW_ERR_INVALID_ARG, "set_stop_check: reserved must be 0");
  h->live.stop = *c;
  h->live.stop_on = true;
  return SFW_OK;
}

int sfw_get_stop_check(sfw_handle h, sfw_stop_check *out, int32_t *active_out) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!out) return fail(h, SFW_ERR_INVALID_ARG, "get_stop_check: null pointer");
  *out = h->live.stop;
  if (active_out) *active_out = h->live.stop_on ? 1 : 0;
  return SFW_OK;
}

int sfw_grid_stop_info(sfw_handle h, int64_t first, int64_t count, sfw_stop_rec *out) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!h->st.valid) return fail(h, SFW_ERR_STATE, "grid_stop_info before grid_stage");
  if (!h->st.stop_on) return fail(h, SFW_ERR_STATE, "grid_stop_info: the staged grid has no stop check (sfw_set_stop_check)");
  if (!h->last.launched) return fail(h, SFW_ERR_STATE, "grid_stop_info before grid_launch");
  const int64_t T = static_cast<int64_t>(h->st.nv) * h->st.nw;
  if (!sample_range_ok(first, count, T) || !out) return fail(h, SFW_ERR_INVALID_ARG, "grid_stop_info: bad range or buffer");
  SFW_HIP(h, hipSetDevice(h->device));
  const size_t n = static_cast<size_t>(count);
  std::vector<int32_t> steps(n), hit(n);
  SFW_HIP(h, hipMemcpyAsync(steps.data(), h->stop_steps.p + first, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
  SFW_HIP(h, hipMemcpyAsync(hit.data(), h->stop_hit.p + first, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
  SFW_HIP(h, hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < n; ++i) out[i] = sfw_stop_rec{steps[i], hit[i]};
  return SFW_OK;
}

int sfw_grid_stop_points(sfw_handle h, int64_t first, int64_t count, int32_t steps_cap, double *points_xyth, int32_t *n_steps) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!h->st.valid) return fail(h, SFW_ERR_STATE, "grid_stop_points before grid_stage");
  if (!h->st.stop_on) return fail(h, SFW_ERR_STATE, "grid_stop_points: the staged grid has no stop check (sfw_set_stop_check)");
  const int64_t T = static_cast<int64_t>(h->st.nv) * h->st.nw;
  if (!sample_range_ok(first, count, T) || steps_cap < 1 || !points_xyth || !n_steps)
    return fail(h, SFW_ERR_INVALID_ARG, "grid_stop_points: bad range, steps_cap < 1 or null buffer");
  SFW_HIP(h, hipSetDevice(h->device));
  if (int e = flush_arena(h)) return e;  // (the re-run below reads the device copy of the arena)
  const size_t n = static_cast<size_t>(count), pts = 3 * static_cast<size_t>(steps_cap) * n;
  // K1 and the tail once more for those samples into scratch outputs, as sfw_grid_points_batch does
  SFW_HIP(h, reserve_scratch(h, count, false));
  SFW_HIP(h, h->stop_pts.reserve(pts));
  sfw_launch L;
  fill_scratch_launch(h, L, first, count, false, false);
  L.stop_points = h->stop_pts.p;
  L.stop_points_cap = steps_cap;
  SFW_HIP(h, hipMemsetAsync(h->stop_pts.p, 0, sizeof(double) * pts, h->stream));  // (poses behind a tail's end: zeros)
  SFW_HIP(h, sfw_launch_rollout(L, h->stream));
  SFW_HIP(h, hipMemcpyAsync(n_steps, h->pts.stop_steps.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
  SFW_HIP(h, hipMemcpyAsync(points_xyth, h->stop_pts.p, sizeof(double) * pts, hipMemcpyDeviceToHost, h->stream));
  SFW_HIP(h, hipStreamSynchronize(h->stream));
  return SFW_OK;
}

int sfw_set_path(sfw_handle h, const sfw_path *p) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!p) {
    h->live.path_on = false;
    h->live.path_weight = 0.0;
    h->live.path_xy.clear();
    return SFW_OK;
  }
  if (!p->xy) return fail(h, SFW_ERR_INVALID_ARG, "set_path: xy is NULL");
  if (p->n_points < 1 || p->n_points > SFW_PATH_MAX_POINTS)
    return fail(h, SFW_ERR_INVALID_ARG, "set_path: n_points outside 1 .. SFW_PATH_MAX_POINTS");
  if (p->reserved != 0) return fail(h, SFW_ERR_INVALID_ARG, "set_path: reserved must be 0");
  if (!std::isfinite(p->weight)) return fail(h, SFW_ERR_INVALID_ARG, "set_path: the weight is not finite");
  for (int32_t i = 0; i < 2 * p->n_points; ++i)
    if (!(std::fabs(p->xy[i]) <= SFW_PATH_MAX_COORD))  // (a NaN fails the comparison too)
      return fail(h, SFW_ERR_INVALID_ARG, "set_path: a coordinate is not finite or beyond SFW_PATH_MAX_COORD");
  h->live.path_xy.assign(p->xy, p->xy + 2 * static_cast<size_t>(p->n_points));
  h->live.path_weight = p->weight;
  h->live.path_on = true;
  return SFW_OK;
}

int sfw_get_path(sfw_handle h, double *xy_out, int32_t cap, int32_t *n_points_out, double *weight_out, int32_t *active_out) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (cap < 0 || (cap > 0 && !xy_out)) return fail(h, SFW_ERR_INVALID_ARG, "get_path: cap < 0, or xy_out is NULL with cap > 0");
  const size_t n = h->live.path_xy.size() / 2;
  if (xy_out && n > 0) std::memcpy(xy_out, h->live.path_xy.data(), sizeof(double) * 2 * std::min(n, static_cast<size_t>(cap)));
  if (n_points_out) *n_points_out = static_cast<int32_t>(n);
  if (weight_out) *weight_out = h->live.path_weight;
  if (active_out) *active_out = h->live.path_on ? 1 : 0;
  return SFW_OK;
}

int sfw_grid_path_term(sfw_handle h, int64_t first, int64_t count, double *out) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!h->st.valid) return fail(h, SFW_ERR_STATE, "grid_path_term before grid_stage");
  if (!h->st.path_on) return fail(h, SFW_ERR_STATE, "grid_path_term: the staged grid has no path (sfw_set_path)");
  if (!h->last.launched) return fail(h, SFW_ERR_STATE, "grid_path_term before grid_launch");
  const int64_t T = static_cast<int64_t>(h->st.nv) * h->st.nw;
  if (!sample_range_ok(first, count, T) || !out) return fail(h, SFW_ERR_INVALID_ARG, "grid_path_term: bad range or buffer");
  SFW_HIP(h, hipSetDevice(h->device));
  SFW_HIP(h, hipMemcpyAsync(out, h->path_p.p + first, sizeof(double) * static_cast<size_t>(count), hipMemcpyDeviceToHost, h->stream));
  SFW_HIP(h, hipStreamSynchronize(h->stream));
  return SFW_OK;
}

int sfw_set_terms_capture(sfw_handle h, int32_t enabled) {
  if (!h) return SFW_ERR_INVALID_ARG;
  h->live.capture_terms = enabled != 0;
  if (!h->live.capture_terms) {
    h->last.terms = false;
    h->st.early_poses_terms = false;
    if (h->terms.p) {
      SFW_HIP(h, hipSetDevice(h->device));
      SFW_HIP(h, hipStreamSynchronize(h->stream));  // (a launch in flight may still be writing there)
      h->terms.release();
    }
  }
  return SFW_OK;
}

}  // extern "C"
namespace {
// sfw_grid_rescore (sweep false: K weight vectors w[0..K), the staged path weight where a path is staged) and
// sfw_grid_rescore_path (sweep true: the one vector *w, K times, under path_weight[0..K) — null: the staged weight)
int rescore_run(sfw_handle h, const char *what_c, const sfw_weights *w, bool sweep, const double *path_weight, int32_t K,
                sfw_best *best_out, double *costs_out) {
  if (!h) return SFW_ERR_INVALID_ARG;
  const std::string what = what_c;
  if (!w || !best_out) return fail(h, SFW_ERR_INVALID_ARG, what + ": weights or best_out is NULL");
  if (K < 1 || K > SFW_RESCORE_MAX_K) return fail(h, SFW_ERR_INVALID_ARG, what + ": K out of [1, SFW_RESCORE_MAX_K]");
  if (!all_finite(reinterpret_cast<const double *>(w), (sweep ? size_t(1) : static_cast<size_t>(K)) * SFW_N_TERMS) ||
      (path_weight && !all_finite(path_weight, static_cast<size_t>(K))))
    return fail(h, SFW_ERR_INVALID_ARG, what + ": non-finite weight");
  if (!h->last.launched || !h->last.terms)
    return fail(h, SFW_ERR_STATE, what + ": the last launch did not capture terms (sfw_set_terms_capture), or a stage or "
                                         "sfw_score_one came in since");
  if (sweep && !h->st.path_on) return fail(h, SFW_ERR_STATE, what + ": the staged grid has no path (sfw_set_path)");
  SFW_HIP(h, hipSetDevice(h->device));
  const bool path = h->st.path_on;
  const int64_t T = static_cast<int64_t>(h->st.nv) * h->st.nw;
  const size_t sel_bytes = (sizeof(sfw_sel) * static_cast<size_t>(K) + 15) & ~size_t(15);
  const size_t w_bytes = sizeof(sfw_weights) * static_cast<size_t>(K);
  const size_t pw_bytes = path ? sizeof(double) * static_cast<size_t>(K) : 0;
  // (growing the pinned area frees the old one: nothing in the stream may still be writing there)
  if (sel_bytes + w_bytes + pw_bytes > h->pin_rescore.cap) SFW_HIP(h, hipStreamSynchronize(h->stream));
  SFW_HIP(h, h->pin_rescore.reserve(sel_bytes + w_bytes + pw_bytes));
  sfw_sel *const sel_host = reinterpret_cast<sfw_sel *>(h->pin_rescore.p);
  if (sweep)
    for (int32_t k = 0; k < K; ++k) std::memcpy(h->pin_rescore.p + sel_bytes + sizeof(sfw_weights) * static_cast<size_t>(k), w, sizeof(sfw_weights));
  else
    std::memcpy(h->pin_rescore.p + sel_bytes, w, w_bytes);
  SFW_HIP(h, h->rescore_w.reserve(static_cast<size_t>(K)));
  SFW_HIP(h, hipMemcpyAsync(h->rescore_w.p, h->pin_rescore.p + sel_bytes, w_bytes, hipMemcpyHostToDevice, h->stream));
  if (path) {  // one path weight per vector, behind the weight vectors
    double *const pw = reinterpret_cast<double *>(h->pin_rescore.p + sel_bytes + w_bytes);
    for (int32_t k = 0; k < K; ++k) pw[k] = path_weight ? path_weight[k] : h->st.path_weight;
    SFW_HIP(h, h->rescore_pw.reserve(static_cast<size_t>(K)));
    SFW_HIP(h, hipMemcpyAsync(h->rescore_pw.p, pw, pw_bytes, hipMemcpyHostToDevice, h->stream));
  }
  // weight vectors per launch: all K, or — with costs_out — as many as 256 MB of device cost vectors hold (each launch's are
  // copied out behind it)
  int32_t k_step = K;
  if (costs_out) {
    const int64_t fit = std::max<int64_t>(1, (int64_t(256) << 20) / (static_cast<int64_t>(sizeof(double)) * T));
    k_step = static_cast<int32_t>(std::min<int64_t>(K, fit));
    SFW_HIP(h, h->rescore_costs.reserve(static_cast<size_t>(k_step) * static_cast<size_t>(T)));
  }
  for (int32_t k0 = 0; k0 < K; k0 += k_step) {
    const int32_t n = std::min(k_step, K - k0);
    const int64_t blocks = sfw_rescore_blocks(T, n);
    SFW_HIP(h, h->rescore_partials.reserve(static_cast<size_t>(blocks) * static_cast<size_t>(n)));
    SFW_HIP(h, sfw_launch_rescore(h->terms.p, T, h->rescore_w.p + k0, n, h->st.d_linvels, h->st.d_angvels, h->st.nw, h->st.index_base,
                                  h->rescore_partials.p, costs_out ? h->rescore_costs.p : nullptr, sel_host + k0, h->stream,
                                  h->st.list, path ? h->path_p.p : nullptr, path ? h->rescore_pw.p + k0 : nullptr));
    if (costs_out)
      SFW_HIP(h, hipMemcpyAsync(costs_out + static_cast<int64_t>(k0) * T, h->rescore_costs.p,
                                sizeof(double) * static_cast<size_t>(n) * static_cast<size_t>(T), hipMemcpyDeviceToHost, h->stream));
  }
  SFW_HIP(h, h->pin_rescore.mark(h->stream));
  SFW_HIP(h, wait_stream(h));
  h->pin_rescore.pending = false;
  for (int32_t k = 0; k < K; ++k)
    if (int e = sel_to_best(h, sel_host[k], best_out + k, nullptr)) return e;
  return SFW_OK;
}
}  // namespace
extern "C" {

int sfw_grid_rescore(sfw_handle h, const sfw_weights *w, int32_t K, sfw_best *best_out, double *costs_out) {
  return rescore_run(h, "grid_rescore", w, false, nullptr, K, best_out, costs_out);
}

int sfw_grid_rescore_path(sfw_handle h, const sfw_weights *w, const double *path_weight, int32_t K, sfw_best *best_out,
                          double *costs_out) {
  return rescore_run(h, "grid_rescore_path", w, true, path_weight, K, best_out, costs_out);
}

int sfw_grid_blend(sfw_handle h, const double *lambda, int32_t L, const double *bias, sfw_blend_stat *stat_out, double *u_out,
                   double *weights_out) {
  return grid_blend(h, "grid_blend", lambda, L, nullptr, bias, stat_out, u_out, weights_out);
}

int sfw_sequences_control_cost(sfw_handle h, double gamma, double *bias_out) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!bias_out || !std::isfinite(gamma)) return fail(h, SFW_ERR_INVALID_ARG, "sequences_control_cost: bias_out is NULL, or gamma is not finite");
  if (const char *why = control_state_refusal(h)) return fail(h, SFW_ERR_STATE, std::string("sequences_control_cost: ") + why);
  SFW_HIP(h, hipSetDevice(h->device));
  const size_t bytes = sizeof(double) * static_cast<size_t>(h->st.nv);
  if (bytes > h->pin_knots.cap) SFW_HIP(h, hipStreamSynchronize(h->stream));  // (growing the area frees the old one)
  SFW_HIP(h, h->pin_knots.reserve(bytes));
  if (int e = control_cost_enqueue(h, gamma, nullptr, nullptr, h->mppi, h->blend)) return e;
  SFW_HIP(h, hipMemcpyAsync(h->pin_knots.p, h->mppi.ctrl_bias.p, bytes, hipMemcpyDeviceToHost, h->stream));
  SFW_HIP(h, wait_stream(h));
  std::memcpy(bias_out, h->pin_knots.p, bytes);
  return SFW_OK;
}

int sfw_grid_blend_control(sfw_handle h, const double *lambda, int32_t L, double gamma, const double *bias, sfw_blend_stat *stat_out,
                           double *u_out, double *weights_out) {
  return grid_blend(h, "grid_blend_control", lambda, L, &gamma, bias, stat_out, u_out, weights_out);
}

int sfw_mppi_run(sfw_handle h, const sfw_robot_state *rs, const sfw_perturb *p, int32_t n, int32_t K, const int32_t *knot_step,
                 const sfw_goal_args *args, const sfw_mppi *m, sfw_blend_stat *stat_out, double *plans_out, sfw_best *best_out) {
  if (!h) return SFW_ERR_INVALID_ARG;
  // (refused before anything is touched: the staged grid, list or sequences stay launchable)
  if (!m || !stat_out || !plans_out) return fail(h, SFW_ERR_INVALID_ARG, "mppi_run: m, stat_out or plans_out is NULL");
  if (const char *why = mppi_refusal(m)) return fail(h, SFW_ERR_INVALID_ARG, std::string("mppi_run: ") + why);
  if (const char *why = perturb_refusal(rs, p, n, K, knot_step, args, 0)) return fail(h, SFW_ERR_INVALID_ARG, std::string("mppi_run: ") + why);
  if (int e = sfw_sequences_perturb_stage(h, rs, p, n, K, knot_step, args, 0)) return e;
  if (int e = mppi_chain(h, p, m, stat_out, plans_out, best_out)) {
    if (h->mppi.pin_mppi.done) (void)h->mppi.pin_mppi.mark(h->stream);  // (kernels of the chain may still be writing there)
    const std::string why = h->err;
    drop_stage(h);
    h->err = why;
    return e;
  }
  return SFW_OK;
}

int sfw_grid_terms(sfw_handle h, int64_t first, int64_t count, double *terms_out) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!h->last.launched || !h->last.terms)
    return fail(h, SFW_ERR_STATE, "grid_terms: the last launch did not capture terms (sfw_set_terms_capture), or a stage or "
                                  "sfw_score_one came in since");
  const int64_t T = static_cast<int64_t>(h->st.nv) * h->st.nw;
  // (an empty range may also sit at the end of the grid)
  if (count == 0 ? first < 0 || first > T : !sample_range_ok(first, count, T))
    return fail(h, SFW_ERR_INVALID_ARG, "grid_terms: range out of the grid");
  if (count > 0 && !terms_out) return fail(h, SFW_ERR_INVALID_ARG, "grid_terms: terms_out is NULL");
  if (count == 0) return SFW_OK;
  SFW_HIP(h, hipSetDevice(h->device));
  std::vector<double> soa(static_cast<size_t>(SFW_N_TERMS) * static_cast<size_t>(count));
  for (int k = 0; k < SFW_N_TERMS; ++k)
    SFW_HIP(h, hipMemcpyAsync(soa.data() + static_cast<size_t>(k) * count, h->terms.p + k * T + first, sizeof(double) * count,
                              hipMemcpyDeviceToHost, h->stream));
  SFW_HIP(h, hipStreamSynchronize(h->stream));
  stream_is_idle(h);
  for (int64_t i = 0; i < count; ++i)
    for (int k = 0; k < SFW_N_TERMS; ++k) terms_out[i * SFW_N_TERMS + k] = soa[static_cast<size_t>(k * count + i)];
  return SFW_OK;
}

int sfw_last_clock_ghz(sfw_handle h, double *ghz_out) {
  if (!h || !ghz_out) return SFW_ERR_INVALID_ARG;
  if (!h->last.launched) return fail(h, SFW_ERR_STATE, "last_clock_ghz before grid_launch");
  if (!h->last.timed) return fail(h, SFW_ERR_STATE, "last_clock_ghz: timing was off for the last launch (sfw_set_timing)");
  SFW_HIP(h, hipSetDevice(h->device));
  SFW_HIP(h, hipEventSynchronize(h->ev[3]));
  unsigned long long v[4] = {0, 0, 0, 0};
  SFW_HIP(h, hipMemcpy(v, h->clock.p, sizeof(v), hipMemcpyDeviceToHost));
  int wall_khz = 0;
  SFW_HIP(h, hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, h->device));
  *ghz_out = 0.0;  // no sample: no agents, or wave 0 had nothing to integrate
  if (v[2] > v[0] && v[3] > v[1] && wall_khz > 0)
    *ghz_out = static_cast<double>(v[2] - v[0]) / static_cast<double>(v[3] - v[1]) * wall_khz * 1e-6;
  return SFW_OK;
}

int sfw_grid_points_batch(sfw_handle h, int64_t first, int64_t count, double *points_xyth, int32_t *n_points) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!h->st.valid) return fail(h, SFW_ERR_STATE, "grid_points before grid_stage");
  const int64_t T = static_cast<int64_t>(h->st.nv) * h->st.nw;
  if (!sample_range_ok(first, count, T) || !points_xyth || !n_points)
    return fail(h, SFW_ERR_INVALID_ARG, "grid_points: bad range or buffer");
  SFW_HIP(h, hipSetDevice(h->device));
  if (int e = flush_arena(h)) return e;  // (a dump between stage and launch: the re-run below reads the device copy of the arena)
  const int S = num_steps_of(h->live.params);
  const size_t n = static_cast<size_t>(count);
  if (h->last.launched && h->last.captured && h->last.cap_S == S) {  // (sfw_set_params since the launch changed the step count: re-run below)
    // the scoring launch left everything in pinned memory (sfw_set_points_capture): points | counts | contact steps, no
    // kernel, no copy — only the wait for the launch, if no fetch has waited for it yet
    const size_t pts_bytes = sizeof(double) * 3 * static_cast<size_t>(S) * static_cast<size_t>(T);
    if (!h->last.fetched) {
      SFW_HIP(h, wait_stream(h));
    }
    const int32_t *np = reinterpret_cast<const int32_t *>(h->pin_cap.p + pts_bytes), *coll = np + T;
    std::memcpy(points_xyth, h->pin_cap.p + sizeof(double) * 3 * static_cast<size_t>(S) * static_cast<size_t>(first), sizeof(double) * 3 * S * n);
    for (size_t i = 0; i < n; ++i) n_points[i] = contact_trim(np[first + static_cast<int64_t>(i)], coll[first + static_cast<int64_t>(i)]);
    return SFW_OK;
  }
  SFW_HIP(h, h->points.reserve(3 * static_cast<size_t>(S) * n));
  SFW_HIP(h, h->n_points.reserve(n));
  // Re-run K1 for those samples into scratch outputs so the grid results stay intact.
  hipError_t e = reserve_scratch(h, count, false);
  if (e == hipSuccess) {
    sfw_launch L;
    fill_scratch_launch(h, L, first, count, false, false);  // (keep the launch's contact steps)
    L.points = h->points.p;
    L.n_points = h->n_points.p;
    e = sfw_launch_rollout(L, h->stream);
  }
  std::vector<int32_t> coll(n, -1);
  // a capturing launch wrote its contact steps into the capture buffer, not into coll_step (this path is then only reached
  // when the step count changed since: cap_S != S): the contact steps come from the re-integration below instead
  const bool coll_elsewhere = h->last.launched && h->last.captured;
  if (e == hipSuccess && h->last.launched && !coll_elsewhere)
    e = hipMemcpyAsync(coll.data(), h->coll_step.p + first, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(n_points, h->n_points.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(points_xyth, h->points.p, sizeof(double) * 3 * S * n, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return hip_fail(h, e, "grid_points");
  // A sample whose footprint turns illegal at pose a was never integrated by the grid launch.  If a pedestrian
  // touches the robot at an earlier step b < a the reference's Trajectory ends there with b + 1 points (ref :613-627
  // return before pose a is reached): integrate the range once more with those samples kept alive and take their
  // contact steps from that run.
  bool rejected = false;
  for (size_t i = 0; i < n && !rejected; ++i) rejected = n_points[i] < S;
  if ((rejected || coll_elsewhere) && h->st.A > 1) {
    if (int rc = check_lds(h, h->st.A, h->st.O, h->st.NG, h->st.n_grp_mem, count)) return rc;
    sfw_launch L;
    fill_scratch_launch(h, L, first, count, false, true);
    L.force_alive = 1;
    SFW_HIP(h, hipMemsetAsync(h->pts.coll.p, 0xff, sizeof(int32_t) * n, h->stream));  // -1: no contact
    SFW_HIP(h, launch_social_of(L, h->stream));
    SFW_HIP(h, hipMemcpyAsync(coll.data(), h->pts.coll.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
    SFW_HIP(h, hipStreamSynchronize(h->stream));
  }
  for (size_t i = 0; i < n; ++i) n_points[i] = contact_trim(n_points[i], coll[i]);
  return SFW_OK;
}

int sfw_grid_points(sfw_handle h, int64_t index, double *points_xyth, int32_t points_cap, int32_t *n_points) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!points_xyth || points_cap <= 0) return fail(h, SFW_ERR_INVALID_ARG, "grid_points: bad index or buffer");
  const int S = num_steps_of(h->live.params);
  std::vector<double> tmp(static_cast<size_t>(3) * S);
  int32_t n = 0;
  if (int rc = sfw_grid_points_batch(h, index, 1, tmp.data(), &n)) return rc;
  const int m = n < points_cap ? n : points_cap;
  std::memcpy(points_xyth, tmp.data(), sizeof(double) * 3 * static_cast<size_t>(m));
  if (n_points) *n_points = n;
  return SFW_OK;
}

void *sfw_stream(sfw_handle h) { return h ? static_cast<void *>(h->stream) : nullptr; }

}  // extern "C"

namespace {
// Sample t of the stage once more, alone, with the crowd capture: K1 into scratch outputs (the re-run of
// sfw_grid_points_batch: the launch's results stay intact), then ONE wave of sfw_crowd_kernel reading the K1 table, then one
// D2H of cost | point count | contact step | rows.  force_alive: a costmap-rejected sample is integrated too and trimmed here
// to the steps the reference integrates before it returns.
int crowd_run(sfw_handle h, int64_t t, double *cost_out, double *state_xyvv, double *work, int32_t *has_goal, int32_t steps_cap,
              int32_t *n_steps) {
  SFW_HIP(h, hipSetDevice(h->device));
  if (int e = flush_arena(h)) return e;  // (the kernels below read the device copy of the arena)
  const int S = num_steps_of(h->live.params), A = h->st.A;
  // check_lds prices the score path, not the crowd wave's own layout; it covers it because sfw_social_lds_bytes always
  // includes the flat form at the score path's plane capacity, and the crowd wave runs the same layout at the run-time
  // capacity (never larger) without the points' LDS copy.  launch_crowd_typed's own limits (160 KiB, 16-bit plane offsets)
  // therefore never refuse what passed here; if its layout ever outgrows the flat form's, price it here, so that the caller
  // sees SFW_ERR_UNSUPPORTED and not a HIP error.
  if (A > 0)
    if (int e = check_lds(h, A, h->st.O, h->st.NG, h->st.n_grp_mem, 1)) return e;
  const size_t SA = static_cast<size_t>(S) * static_cast<size_t>(A);
  const size_t head = 16, o_work = head + sizeof(double) * 4 * SA, o_hg = o_work + sizeof(double) * SA,
               total = o_hg + sizeof(int32_t) * SA;
  SFW_HIP(h, h->crowd_out.reserve(total));
  SFW_HIP(h, reserve_scratch(h, 1, true));
  if (A > 0 && h->crowd_pair_tab_A != A) {
    h->crowd_pair_tab_A = -1;  // (until the table for this count is enqueued)
    SFW_HIP(h, h->crowd_pair_tab.reserve(static_cast<size_t>(sfw_pair_table_entries(A))));
    SFW_HIP(h, sfw_launch_pair_table(h->crowd_pair_tab.p, A, h->stream, true));
    h->crowd_pair_tab_A = A;
  }
  char *const out = h->crowd_out.p;
  sfw_launch L;
  fill_scratch_launch(h, L, t, 1, true, false);  // (with the path term: the sample's cost carries it)
  L.costs = reinterpret_cast<double *>(out) - t;
  L.coll_step = reinterpret_cast<int32_t *>(out + 12) - t;
  L.n_points = reinterpret_cast<int32_t *>(out + 8);
  L.pair_tab = h->crowd_pair_tab.p;
  L.force_alive = 1;
  SFW_HIP(h, sfw_launch_rollout(L, h->stream));
  if (A > 0) {
    const sfw_crowd_out cw{reinterpret_cast<double *>(out + head), reinterpret_cast<double *>(out + o_work),
                           reinterpret_cast<int32_t *>(out + o_hg)};
    SFW_HIP(h, h->live.params.precision == SFW_PRECISION_F64_STRICT ? sfw_launch_crowd_strict(L, cw, h->stream)
                                                                     : sfw_launch_crowd(L, cw, h->stream));
  }
  if (L.path_on) SFW_HIP(h, sfw_launch_path_add(L.costs, L.path_p, h->st.path_weight, t, 1, h->stream));
  SFW_HIP(h, h->pin_crowd.reserve(total));
  SFW_HIP(h, hipMemcpyAsync(h->pin_crowd.p, out, total, hipMemcpyDeviceToHost, h->stream));
  SFW_HIP(h, hipStreamSynchronize(h->stream));
  const char *const pin = h->pin_crowd.p;
  int32_t n = one_head_unpack(pin, cost_out);
  if (A <= 0) n = 0;  // nobody to predict
  *n_steps = n;
  const size_t m = static_cast<size_t>(n < steps_cap ? n : steps_cap) * static_cast<size_t>(A > 0 ? A : 0);
  if (m > 0) {
    std::memcpy(state_xyvv, pin + head, sizeof(double) * 4 * m);
    if (work) std::memcpy(work, pin + o_work, sizeof(double) * m);
    if (has_goal) std::memcpy(has_goal, pin + o_hg, sizeof(int32_t) * m);
  }
  return SFW_OK;
}
}  // namespace

extern "C" {

int sfw_score_one_crowd(sfw_handle h, const sfw_robot_state *rs, double vx_samp, double vy_samp, double vtheta_samp,
                        const sfw_goal_args *args, double *cost_out, double *state_xyvv, double *work, int32_t *has_goal,
                        int32_t agents, int32_t steps_cap, int32_t *n_steps) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!cost_out || !state_xyvv || !n_steps || steps_cap < 1)
    return fail(h, SFW_ERR_INVALID_ARG, "score_one_crowd: cost_out, state_xyvv or n_steps is NULL, or steps_cap < 1");
  if (agents != h->world.agents.A) return fail(h, SFW_ERR_INVALID_ARG, "score_one_crowd: agents is not the agent count of sfw_set_agents");
  if (int e = stage_one(h, rs, args, vx_samp, vy_samp, vtheta_samp)) return e;
  consume_stage consumed{h};
  return crowd_run(h, 0, cost_out, state_xyvv, work, has_goal, steps_cap, n_steps);
}

int sfw_grid_crowd(sfw_handle h, int64_t index, double *cost_out, double *state_xyvv, double *work, int32_t *has_goal,
                   int32_t agents, int32_t steps_cap, int32_t *n_steps) {
  if (!h) return SFW_ERR_INVALID_ARG;
  if (!state_xyvv || !n_steps || steps_cap < 1)
    return fail(h, SFW_ERR_INVALID_ARG, "grid_crowd: state_xyvv or n_steps is NULL, or steps_cap < 1");
  if (!h->st.valid) return fail(h, SFW_ERR_STATE, "grid_crowd before grid_stage");
  const int64_t T = static_cast<int64_t>(h->st.nv) * h->st.nw;
  if (index < 0 || index >= T) return fail(h, SFW_ERR_INVALID_ARG, "grid_crowd: bad index");
  if (agents != h->st.A) return fail(h, SFW_ERR_INVALID_ARG, "grid_crowd: agents is not the agent count of the staged world");
  return crowd_run(h, index, cost_out, state_xyvv, work, has_goal, steps_cap, n_steps);
}

}  // extern "C"

// ===========================================================================
// one process, several devices (sfw_multi_*)
// ===========================================================================
namespace {
// The six RCCL entry points this file uses, declared here (values as in <rccl/rccl.h> of ROCm 7.2, NCCL 2.x ABI) so
// that the library builds on a ROCm install without the rccl development package and a single-device caller never
// needs librccl at all: it is resolved with dlopen on the first sfw_multi_create(SFW_MULTI_RCCL).
typedef struct ncclComm *ncclComm_t;
typedef int ncclResult_t;
constexpr ncclResult_t ncclSuccess = 0;
constexpr int ncclDouble = 8;  // ncclDataType_t: ncclFloat64
constexpr int ncclMin = 3;     // ncclRedOp_t
struct rccl_api {
  void *lib = nullptr;
  std::string error;
  ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  // optional (sfw_multi_describe): what the communicators say about themselves
  ncclResult_t (*GetVersion)(int *) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
  ncclResult_t (*CommCuDevice)(const ncclComm_t, int *) = nullptr;
  std::string path;      // the file ncclAllReduce really came from (dladdr)
  std::string how;       // "SFW_RCCL_LIB", "already mapped", or the name dlopen was given
  // Which RCCL?  (1) SFW_RCCL_LIB in the environment: that file, or an error — never a silent fall-through; (2) an RCCL
  // this process has mapped already (a Python process that imported torch holds torch's bundled copy: a second RCCL beside
  // it would mean two sets of communicator state in one process) — found by walking the loaded objects, reopened with
  // RTLD_NOLOAD; (3) the loader's search: librccl.so, librccl.so.1, /opt/rocm/lib/librccl.so.
  void load_once() {
    if (const char *forced = std::getenv("SFW_RCCL_LIB")) {
      if (forced[0]) {
        lib = dlopen(forced, RTLD_NOW | RTLD_LOCAL);
        if (!lib) {
          error = std::string("SFW_RCCL_LIB=") + forced + ": " + dlerror();
          return;
        }
        how = "SFW_RCCL_LIB";
      }
    }
    if (!lib) {
      std::string mapped;
      dl_iterate_phdr(
          [](struct dl_phdr_info *info, size_t, void *out) {
            if (info->dlpi_name && std::strstr(info->dlpi_name, "librccl.so")) {
              *static_cast<std::string *>(out) = info->dlpi_name;
              return 1;
            }
            return 0;
          },
          &mapped);
      if (!mapped.empty()) {
        lib = dlopen(mapped.c_str(), RTLD_NOW | RTLD_NOLOAD | RTLD_LOCAL);
        if (lib) how = "already mapped";
      }
    }
    if (!lib)
      for (const char *name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
        lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (lib) {
          how = name;
          break;
        }
      }
    if (!lib) {
      error = std::string("cannot load librccl.so: ") + dlerror();
      return;
    }
    auto sym = [&](const char *n) { return dlsym(lib, n); };
    CommInitAll = reinterpret_cast<decltype(CommInitAll)>(sym("ncclCommInitAll"));
    CommDestroy = reinterpret_cast<decltype(CommDestroy)>(sym("ncclCommDestroy"));
    AllReduce = reinterpret_cast<decltype(AllReduce)>(sym("ncclAllReduce"));
    GroupStart = reinterpret_cast<decltype(GroupStart)>(sym("ncclGroupStart"));
    GroupEnd = reinterpret_cast<decltype(GroupEnd)>(sym("ncclGroupEnd"));
    GetErrorString = reinterpret_cast<decltype(GetErrorString)>(sym("ncclGetErrorString"));
    GetVersion = reinterpret_cast<decltype(GetVersion)>(sym("ncclGetVersion"));
    CommCount = reinterpret_cast<decltype(CommCount)>(sym("ncclCommCount"));
    CommCuDevice = reinterpret_cast<decltype(CommCuDevice)>(sym("ncclCommCuDevice"));
    if (!CommInitAll || !CommDestroy || !AllReduce || !GroupStart || !GroupEnd || !GetErrorString) {
      dlclose(lib);
      lib = nullptr;
      error = "librccl.so lacks ncclCommInitAll/ncclAllReduce/ncclGroupStart/...";
      return;
    }
    Dl_info di;
    if (dladdr(reinterpret_cast<void *>(AllReduce), &di) && di.dli_fname) path = di.dli_fname;
  }
  // "" or why RCCL is not available; safe from several threads (two planners created concurrently)
  const std::string &load() {
    std::call_once(once, [this] { load_once(); });
    return error;
  }
  std::once_flag once;
};
rccl_api g_rccl;
thread_local std::string g_multi_create_error;

// One worker thread per rank of a multi handle, alive for the handle's lifetime: a rank's stage + launch is ~100 us
// of host work (shared-prefix planning, one H2D copy, a dozen kernel launches) and the ranks are independent, so a
// grid cut R ways is enqueued in the time of one rank instead of R.  run() hands every worker its job and returns
// when all are done.
struct rank_workers {
  struct slot {
    std::thread th;
    std::function<int()> job;
    bool has_job = false, quit = false;
    int rc = 0;
  };
  std::mutex mu;
  std::condition_variable cv_job, cv_done;
  std::vector<slot> w;
  int pending = 0;
  void start(int R) {
    w.resize(static_cast<size_t>(R));
    for (int r = 0; r < R; ++r) w[static_cast<size_t>(r)].th = std::thread([this, r] { loop(r); });
  }
  void loop(int r) {
    slot &me = w[static_cast<size_t>(r)];
    for (;;) {
      std::function<int()> job;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv_job.wait(lk, [&] { return me.has_job || me.quit; });
        if (me.quit) return;
        job = std::move(me.job);
        me.has_job = false;
      }
      const int rc = job();
      {
        std::lock_guard<std::mutex> lk(mu);
        me.rc = rc;
        if (--pending == 0) cv_done.notify_all();
      }
    }
  }
  // jobs[r] runs on worker r; returns the first non-zero result (by rank), or 0
  int run(std::vector<std::function<int()>> &jobs, int *failed_rank) {
    {
      std::lock_guard<std::mutex> lk(mu);
      pending = static_cast<int>(jobs.size());
      for (size_t r = 0; r < jobs.size(); ++r) {
        w[r].job = std::move(jobs[r]);
        w[r].has_job = true;
      }
    }
    cv_job.notify_all();
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [&] { return pending == 0; });
    for (size_t r = 0; r < w.size(); ++r)
      if (w[r].rc != 0) {
        if (failed_rank) *failed_rank = static_cast<int>(r);
        return w[r].rc;
      }
    return 0;
  }
  void stop() {
    {
      std::lock_guard<std::mutex> lk(mu);
      for (slot &s : w) s.quit = true;
    }
    cv_job.notify_all();
    for (slot &s : w)
      if (s.th.joinable()) s.th.join();
    w.clear();
  }
};
}  // namespace

struct sfw_multi_s {
  int R = 0;
  int exchange = SFW_MULTI_RCCL;
  std::vector<sfw_handle> h;
  std::vector<int> dev;
  std::vector<ncclComm_t> comm;       // RCCL exchange only
  std::vector<double *> d_table;      // per rank: [R,5] doubles on its device
  double *pin_table = nullptr;        // pinned host copy: the reduced table (RCCL) or the ranks' own rows (host reduce)
  std::vector<int32_t> row0;          // R + 1 row offsets of the last grid
  std::vector<double> lin, ang;
  int32_t nv = 0, nw = 0;
  bool scored = false;
  double us[3] = {0, 0, 0};
  std::string err;
  rank_workers workers;               // R > 1 only
  std::vector<std::string> rank_err;  // what went wrong on a rank's worker (its handle's message, or a HIP error)
};

#define SFW_MHIP(m, h, call)                                                                  \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      (m)->err = std::string(#call) + ": " + hipGetErrorString(e_);                           \
      return hip_fail((h), e_, #call);                                                        \
    }                                                                                         \
  } while (0)

namespace {
int mfail(sfw_multi_handle m, int code, const std::string &msg) {
  if (m) m->err = msg;
  return code;
}
int mrank_fail(sfw_multi_handle m, int r, int code, const char *what) {
  return mfail(m, code, std::string(what) + " on rank " + std::to_string(r) + ": " + sfw_last_error(m->h[static_cast<size_t>(r)]));
}
double now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
}  // namespace

extern "C" {

int sfw_multi_create(const sfw_params *params, const int *devices, int32_t R, int32_t exchange, sfw_multi_handle *out) {
  if (!out) return SFW_ERR_INVALID_ARG;
  *out = nullptr;
  if (!params || !devices || R <= 0 || R > 64 || (exchange != SFW_MULTI_RCCL && exchange != SFW_MULTI_HOST_REDUCE))
    return SFW_ERR_INVALID_ARG;
  if (exchange == SFW_MULTI_RCCL)
    for (int a = 0; a < R; ++a)
      for (int b = a + 1; b < R; ++b)
        if (devices[a] == devices[b]) return SFW_ERR_INVALID_ARG;  // one RCCL rank per device
  sfw_multi_handle m = new (std::nothrow) sfw_multi_s();
  if (!m) return SFW_ERR_HIP;
  m->R = R;
  m->exchange = exchange;
  m->dev.assign(devices, devices + R);
  m->d_table.assign(static_cast<size_t>(R), nullptr);
  m->rank_err.assign(static_cast<size_t>(R), "");
  int rc = SFW_OK;
  for (int r = 0; r < R && rc == SFW_OK; ++r) {
    sfw_handle h = nullptr;
    rc = sfw_create(params, devices[r], &h);
    if (rc == SFW_OK) {
      m->h.push_back(h);
      if (hipSetDevice(devices[r]) != hipSuccess ||
          hipMalloc(reinterpret_cast<void **>(&m->d_table[static_cast<size_t>(r)]), sizeof(double) * 5 * R) != hipSuccess)
        rc = SFW_ERR_HIP;
    }
  }
  if (rc == SFW_OK && hipHostMalloc(reinterpret_cast<void **>(&m->pin_table), sizeof(double) * 5 * R, hipHostMallocDefault) != hipSuccess)
    rc = SFW_ERR_HIP;
  if (rc == SFW_OK && exchange == SFW_MULTI_RCCL) {
    if (!g_rccl.load().empty()) {
      rc = SFW_ERR_UNSUPPORTED;
      g_multi_create_error = g_rccl.load();
    } else {
      m->comm.assign(static_cast<size_t>(R), nullptr);
      const ncclResult_t nr = g_rccl.CommInitAll(m->comm.data(), R, devices);
      if (nr != ncclSuccess) {
        m->comm.clear();
        rc = SFW_ERR_HIP;
        g_multi_create_error = std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(nr) + " (" + g_rccl.path + ")";
      }
    }
  }
  if (rc != SFW_OK) {
    sfw_multi_destroy(m);
    return rc;
  }
  if (R > 1) m->workers.start(R);
  *out = m;
  return SFW_OK;
}

int sfw_multi_destroy(sfw_multi_handle m) {
  if (!m) return SFW_OK;
  m->workers.stop();
  for (size_t r = 0; r < m->h.size(); ++r) (void)sfw_grid_sync(m->h[r]);
  for (ncclComm_t c : m->comm)
    if (c) (void)g_rccl.CommDestroy(c);
  for (size_t r = 0; r < m->d_table.size(); ++r)
    if (m->d_table[r]) {
      (void)hipSetDevice(m->dev[r]);
      (void)hipFree(m->d_table[r]);
    }
  if (m->pin_table) (void)hipHostFree(m->pin_table);
  for (sfw_handle h : m->h) (void)sfw_destroy(h);
  delete m;
  return SFW_OK;
}

// (a NULL handle: why this thread's last sfw_multi_create failed, when it said why — RCCL could not be resolved or initialised)
const char *sfw_multi_last_error(sfw_multi_handle m) {
  if (m) return m->err.c_str();
  return g_multi_create_error.empty() ? "null handle" : g_multi_create_error.c_str();
}
int32_t sfw_multi_ranks(sfw_multi_handle m) { return m ? m->R : 0; }
int sfw_multi_describe(sfw_multi_handle m, sfw_multi_desc *out) {
  if (!m || !out) return SFW_ERR_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  out->ranks = m->R;
  out->exchange = m->exchange;
  for (int r = 0; r < m->R && r < 64; ++r) out->devices[r] = m->dev[static_cast<size_t>(r)];
  for (int r = 0; r < 64; ++r) out->comm_devices[r] = -1;
  out->comm_size = -1;
  if (m->exchange == SFW_MULTI_RCCL) {
    if (g_rccl.GetVersion) (void)g_rccl.GetVersion(&out->rccl_version);
    std::snprintf(out->rccl_path, sizeof(out->rccl_path), "%s", g_rccl.path.c_str());
    std::snprintf(out->rccl_found, sizeof(out->rccl_found), "%s", g_rccl.how.c_str());
    for (size_t r = 0; r < m->comm.size() && r < 64; ++r)
      if (m->comm[r]) {
        out->communicators += 1;
        if (g_rccl.CommCuDevice) (void)g_rccl.CommCuDevice(m->comm[r], &out->comm_devices[r]);
        if (r == 0 && g_rccl.CommCount) (void)g_rccl.CommCount(m->comm[r], &out->comm_size);
      }
  }
  return SFW_OK;
}
sfw_handle sfw_multi_rank_handle(sfw_multi_handle m, int32_t r) {
  return (m && r >= 0 && r < m->R) ? m->h[static_cast<size_t>(r)] : nullptr;
}

int sfw_multi_set_params(sfw_multi_handle m, const sfw_params *params) {
  if (!m) return SFW_ERR_INVALID_ARG;
  for (int r = 0; r < m->R; ++r)
    if (int e = sfw_set_params(m->h[static_cast<size_t>(r)], params)) return mrank_fail(m, r, e, "sfw_set_params");
  return SFW_OK;
}
int sfw_multi_set_costmap(sfw_multi_handle m, const uint8_t *cells, uint32_t size_x, uint32_t size_y, double origin_x,
                          double origin_y, double resolution) {
  if (!m) return SFW_ERR_INVALID_ARG;
  for (int r = 0; r < m->R; ++r)
    if (int e = sfw_set_costmap(m->h[static_cast<size_t>(r)], cells, size_x, size_y, origin_x, origin_y, resolution))
      return mrank_fail(m, r, e, "sfw_set_costmap");
  return SFW_OK;
}
int sfw_multi_set_footprint(sfw_multi_handle m, const double *xy, int32_t K) {
  if (!m) return SFW_ERR_INVALID_ARG;
  for (int r = 0; r < m->R; ++r)
    if (int e = sfw_set_footprint(m->h[static_cast<size_t>(r)], xy, K)) return mrank_fail(m, r, e, "sfw_set_footprint");
  return SFW_OK;
}
int sfw_multi_set_agents(sfw_multi_handle m, const sfw_agent *agents, int32_t A, const double *obstacles_xy, int32_t O) {
  if (!m) return SFW_ERR_INVALID_ARG;
  // validated, packed and scanned for w x diff == 0 pairs ONCE (the scan is all pairs); the other ranks take rank 0's
  // host-side copy — the upload happens per rank with its next stage
  sfw_handle h0 = m->h[0];
  if (int e = sfw_set_agents(h0, agents, A, obstacles_xy, O)) return mrank_fail(m, 0, e, "sfw_set_agents");
  for (int r = 1; r < m->R; ++r) m->h[static_cast<size_t>(r)]->world.agents = h0->world.agents;
  return SFW_OK;
}

int sfw_multi_score_grid(sfw_multi_handle m, const sfw_robot_state *rs, const double *linvels, int32_t nv,
                         const double *angvels, int32_t nw, const sfw_goal_args *args, double *costs_out,
                         sfw_best *best_out) {
  if (!m) return SFW_ERR_INVALID_ARG;
  if (!rs || !linvels || !angvels || !args || nv <= 0 || nw <= 0)
    return mfail(m, SFW_ERR_INVALID_ARG, "multi_score_grid: null pointer or non-positive sample count");
  const int R = m->R;
  m->scored = false;
  m->lin.assign(linvels, linvels + nv);
  m->ang.assign(angvels, angvels + nw);
  m->nv = nv;
  m->nw = nw;
  const double t0 = now_us();
  sfw_handle h0 = m->h[0];
  if (!all_finite(linvels, static_cast<size_t>(nv)) || !all_finite(angvels, static_cast<size_t>(nw)) || !all_finite(&rs->x, 6) ||
      !all_finite(&args->acc_x, 5))
    return mfail(m, SFW_ERR_INVALID_ARG, "multi_score_grid: non-finite robot state, goal argument or sample velocity");
  {  // ref :345: rows are the outer axis — contiguous blocks of equal planned work (equal row counts when nothing is shared)
    const int S = num_steps_of(h0->live.params);
    const bool sharing = h0->cfg.prefix_env.empty() || h0->cfg.prefix_env[0] != 0;
    plan_row_blocks(m->lin, m->ang, rs->vx, rs->vtheta, args->acc_x, args->acc_theta, h0->live.params.sim_time / S, S, sharing ? h0->world.agents.A : 0, R,
                    h0->live.k2_form, h0->cfg.n_cu, m->row0);
  }
  // (0) what is the same for every rank, once: the agent set must fit a wave's LDS for every rank's item count
  // before anything is launched anywhere, and the classes of the column axis (every rank scores all nw columns)
  for (int r = 0; r < R; ++r) {
    const int64_t items = static_cast<int64_t>(m->row0[static_cast<size_t>(r) + 1] - m->row0[static_cast<size_t>(r)]) * nw;
    if (items > 0 && h0->world.agents.A > 0 && sfw_social_lds_bytes(h0->world.agents.A, h0->world.agents.O, h0->world.agents.NG, h0->world.agents.n_grp_mem, items, h0->live.k2_form, h0->cfg.n_cu) > 160 * 1024)
      return mfail(m, SFW_ERR_UNSUPPORTED, "agent/obstacle set does not fit the 160 KiB LDS of one CU");
  }
  axis_classes cols;
  const axis_classes *shared = nullptr;
  {
    const int S = num_steps_of(h0->live.params);
    const int64_t rows_max = (nv + R - 1) / R;
    if (R > 1 && h0->world.agents.A >= 2 && S >= 2 && rows_max * nw >= 4096 && (h0->cfg.prefix_env.empty() || h0->cfg.prefix_env[0] != 0)) {
      cols = classes_of_axis(m->ang, rs->vtheta, args->acc_theta, h0->live.params.sim_time / S, prefix_max_p(S));
      cols.complete();  // (read by every rank's thread: no level is written lazily from there)
      shared = &cols;
    }
  }
  // (1) every rank: stage its block of rows, enqueue the kernels and its row of the exchange table
  auto rank_job = [&](int r) -> int {
    sfw_handle h = m->h[static_cast<size_t>(r)];
    std::string &err = m->rank_err[static_cast<size_t>(r)];
    err.clear();
    const int32_t lo = m->row0[static_cast<size_t>(r)], n = m->row0[static_cast<size_t>(r) + 1] - lo;
    hipError_t e = hipSetDevice(m->dev[static_cast<size_t>(r)]);
    if (e != hipSuccess) {
      err = std::string("hipSetDevice: ") + hipGetErrorString(e);
      return SFW_ERR_HIP;
    }
    if (n > 0) {
      h->shared_cols = shared;
      const int rc_stage = sfw_grid_stage(h, rs, linvels + lo, n, angvels, nw, args, static_cast<int64_t>(lo) * nw);
      h->shared_cols = nullptr;
      if (rc_stage) {
        err = std::string("sfw_grid_stage: ") + sfw_last_error(h);
        return rc_stage;
      }
      if (int rc = sfw_grid_launch(h)) {
        err = std::string("sfw_grid_launch: ") + sfw_last_error(h);
        return rc;
      }
    }
    // fewer rows than ranks: this rank holds nothing, its row is +inf / 0 valid (null selection record)
    e = sfw_launch_key_table(n > 0 ? h->st.d_sel : nullptr, m->d_table[static_cast<size_t>(r)], r, R, h->stream);
    if (e != hipSuccess) {
      err = std::string("key table launch: ") + hipGetErrorString(e);
      return SFW_ERR_HIP;
    }
    return SFW_OK;
  };
  {
    int failed = 0, rc = SFW_OK;
    if (R == 1) {
      rc = rank_job(0);
    } else {
      std::vector<std::function<int()>> jobs;
      for (int r = 0; r < R; ++r) jobs.emplace_back([&rank_job, r] { return rank_job(r); });
      rc = m->workers.run(jobs, &failed);
    }
    if (rc != SFW_OK) return mfail(m, rc, m->rank_err[static_cast<size_t>(failed)] + " (rank " + std::to_string(failed) + ")");
  }
  const double t1 = now_us();
  // (2) the exchange
  if (m->exchange == SFW_MULTI_RCCL) {
    ncclResult_t nr = g_rccl.GroupStart();
    for (int r = 0; r < R && nr == ncclSuccess; ++r) {
      (void)hipSetDevice(m->dev[static_cast<size_t>(r)]);
      double *t = m->d_table[static_cast<size_t>(r)];
      nr = g_rccl.AllReduce(t, t, static_cast<size_t>(5) * R, ncclDouble, ncclMin, m->comm[static_cast<size_t>(r)],
                            m->h[static_cast<size_t>(r)]->stream);
    }
    const ncclResult_t ne = g_rccl.GroupEnd();
    if (nr == ncclSuccess) nr = ne;
    if (nr != ncclSuccess) return mfail(m, SFW_ERR_HIP, std::string("ncclAllReduce: ") + g_rccl.GetErrorString(nr));
    SFW_MHIP(m, h0, hipSetDevice(m->dev[0]));
    SFW_MHIP(m, h0, hipMemcpyAsync(m->pin_table, m->d_table[0], sizeof(double) * 5 * R, hipMemcpyDeviceToHost, h0->stream));
    SFW_MHIP(m, h0, hipStreamSynchronize(h0->stream));
  } else {  // host reduce: each rank's own row
    for (int r = 0; r < R; ++r) {
      sfw_handle h = m->h[static_cast<size_t>(r)];
      SFW_MHIP(m, h, hipSetDevice(m->dev[static_cast<size_t>(r)]));
      SFW_MHIP(m, h, hipMemcpyAsync(m->pin_table + 5 * r, m->d_table[static_cast<size_t>(r)] + 5 * r, sizeof(double) * 5,
                                hipMemcpyDeviceToHost, h->stream));
    }
    for (int r = 0; r < R; ++r) {
      sfw_handle h = m->h[static_cast<size_t>(r)];
      SFW_MHIP(m, h, hipSetDevice(m->dev[static_cast<size_t>(r)]));
      SFW_MHIP(m, h, hipStreamSynchronize(h->stream));
    }
  }
  const double t2 = now_us();
  // (3) cost slices
  if (costs_out)
    for (int r = 0; r < R; ++r) {
      const int32_t lo = m->row0[static_cast<size_t>(r)], n = m->row0[static_cast<size_t>(r) + 1] - lo;
      if (n > 0)
        if (int e = sfw_grid_fetch(m->h[static_cast<size_t>(r)], costs_out + static_cast<int64_t>(lo) * nw, nullptr, nullptr))
          return mrank_fail(m, r, e, "sfw_grid_fetch");
    }
  const double t3 = now_us();
  m->us[0] = t1 - t0;
  m->us[1] = t2 - t1;
  m->us[2] = t3 - t2;
  // (4) lexicographic minimum over the rows = the reference's selection order
  if (best_out) {
    int win = -1;
    int64_t n_valid = 0;
    for (int r = 0; r < R; ++r) {
      const double *k = m->pin_table + 5 * r;
      n_valid += static_cast<int64_t>(k[4]);
      if (!std::isfinite(k[0])) continue;
      if (win < 0 || std::lexicographical_compare(k, k + 4, m->pin_table + 5 * win, m->pin_table + 5 * win + 4)) win = r;
    }
    best_out->n_valid = n_valid;
    if (win >= 0) {
      const double *k = m->pin_table + 5 * win;
      const int64_t idx = static_cast<int64_t>(-k[3]);
      best_out->index = idx;
      best_out->cost = k[0];
      best_out->vx = linvels[idx / nw];
      best_out->vy = 0.0;
      best_out->vtheta = angvels[idx % nw];
    } else {  // ref :456-468
      best_out->index = -1;
      best_out->cost = -1.0;
      best_out->vx = best_out->vy = best_out->vtheta = 0.0;
    }
  }
  m->scored = true;
  return SFW_OK;
}

int sfw_multi_rank_rows(sfw_multi_handle m, int32_t r, int32_t *first_row, int32_t *n_rows) {
  if (!m || r < 0 || r >= m->R || !first_row || !n_rows) return SFW_ERR_INVALID_ARG;
  if (!m->scored) return mfail(m, SFW_ERR_STATE, "multi_rank_rows before multi_score_grid");
  *first_row = m->row0[static_cast<size_t>(r)];
  *n_rows = m->row0[static_cast<size_t>(r) + 1] - m->row0[static_cast<size_t>(r)];
  return SFW_OK;
}

int sfw_multi_last_us(sfw_multi_handle m, int32_t which, double *us_out) {
  if (!m || !us_out || which < 0 || which > 2) return SFW_ERR_INVALID_ARG;
  if (!m->scored) return mfail(m, SFW_ERR_STATE, "multi_last_us before multi_score_grid");
  *us_out = m->us[which];
  return SFW_OK;
}

int sfw_multi_grid_points(sfw_multi_handle m, int64_t index, double *points_xyth, int32_t points_cap, int32_t *n_points) {
  if (!m) return SFW_ERR_INVALID_ARG;
  if (!m->scored) return mfail(m, SFW_ERR_STATE, "multi_grid_points before multi_score_grid");
  if (index < 0 || index >= static_cast<int64_t>(m->nv) * m->nw) return mfail(m, SFW_ERR_INVALID_ARG, "multi_grid_points: bad index");
  const int32_t row = static_cast<int32_t>(index / m->nw);
  int r = 0;
  while (r + 1 < m->R && row >= m->row0[static_cast<size_t>(r) + 1]) ++r;
  const int64_t local = index - static_cast<int64_t>(m->row0[static_cast<size_t>(r)]) * m->nw;
  if (int e = sfw_grid_points(m->h[static_cast<size_t>(r)], local, points_xyth, points_cap, n_points))
    return mrank_fail(m, r, e, "sfw_grid_points");
  return SFW_OK;
}

}  // extern "C"

// ===========================================================================
// many handles' control cycles in one launch (sfw_batch_*)
// ===========================================================================
struct sfw_batch_s {
  int device = 0;
  hipStream_t stream = nullptr, side = nullptr;  // shared by every member
  std::vector<sfw_handle> h;
  std::string err;
  // the member table of a launch (sfw_device.h sfw_batch_rec): built in pinned memory, ONE H2D copy per launch
  pinned_buf pin_table;
  dev_buf<char> table;
  sfw_batch_desc desc{};
  double us[3] = {0.0, 0.0, 0.0};
  bool launched = false;
  // sfw_batch_set_list_fusion: list / sequence / perturbed members that qualify join the member table (off: their own path)
  bool list_fusion = false;
  // the member table as last uploaded (host copy), and how many uploads there have been: a launch that may re-use the device
  // copy (batch_enqueue reuse_table) compares what it has built with it
  std::vector<char> table_host, table_sent;
  int64_t table_uploads = 0;
};

namespace {
int bfail(sfw_batch b, int code, const std::string &msg) {
  if (b) b->err = msg;
  return code;
}
int bmember_fail(sfw_batch b, int32_t i, int code, const char *what) {
  return bfail(b, code, std::string(what) + " (member " + std::to_string(i) + "): " + b->h[static_cast<size_t>(i)]->err);
}
double us_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
}

// every member staged (batch_launch has checked): one launch per kernel variant for the members that qualify for the
// one-kernel control cycle, the others' kernels behind them on the same stream.  reuse_table (sfw_ensemble_mppi_run, iterations
// > 0): when the table built here is byte for byte the one the device holds, neither the pinned copy — whose reserve waits for
// the last upload's event — nor the upload is redone; when it is not, it is uploaded as always.
int batch_enqueue(sfw_batch b, bool reuse_table = false) {
  const int32_t B = static_cast<int32_t>(b->h.size());
  if (hipSetDevice(b->device) != hipSuccess) return bfail(b, SFW_ERR_HIP, "batch_launch: hipSetDevice failed");
  std::vector<launch_prep> lp(static_cast<size_t>(B));
  std::vector<sfw_launch> L(static_cast<size_t>(B));
  std::vector<int> variant(static_cast<size_t>(B), -1);  // -1: the member's own path
  int32_t n_cycle = 0;
  for (int32_t i = 0; i < B; ++i) {
    const size_t m = static_cast<size_t>(i);
    if (int e = launch_prepare(b->h[m], false, lp[m])) return bmember_fail(b, i, e, "batch_launch");
    // a sample list (sfw_samples_stage, sequences, perturbed rollouts) takes its own path unless the batch fuses lists
    // (sfw_batch_set_list_fusion): then it joins the table under the variant of its kind
    if (b->h[m]->st.list && !b->list_fusion) continue;
    if (cycle_launch_of(b->h[m], lp[m], L[m])) {
      variant[m] = sfw_cycle_batch_variant(L[m]);
      ++n_cycle;
    }
  }
  sfw_batch_desc d{};
  d.members = B;
  d.one_launch_members = n_cycle;
  d.own_path_members = B - n_cycle;
  if (n_cycle > 0) {
    // table: per variant (= per launch) first[n + 1], then the records of all launches, in variant order
    constexpr int kVariants = SFW_BATCH_VARIANTS;
    int32_t count[kVariants] = {};
    for (int v : variant)
      if (v >= 0) ++count[v];
    size_t head = 0;
    size_t first_at[kVariants] = {};
    for (int v = 0; v < kVariants; ++v)
      if (count[v] > 0) {
        first_at[v] = head;
        head += sizeof(uint32_t) * (static_cast<size_t>(count[v]) + 1);
      }
    head = (head + 15) & ~size_t(15);
    const size_t bytes = head + sizeof(sfw_batch_rec) * static_cast<size_t>(n_cycle);
    // (built in plain host memory first: whether it must be uploaded is known only once it stands)
    b->table_host.assign(bytes, 0);
    char *const pt = b->table_host.data();
    size_t rec_at[kVariants] = {};
    for (int v = 0, r = 0; v < kVariants; ++v)
      if (count[v] > 0) {
        rec_at[v] = head + sizeof(sfw_batch_rec) * static_cast<size_t>(r);
        r += count[v];
      }
    int32_t filled[kVariants] = {};
    uint32_t blocks[kVariants] = {};
    size_t lds[kVariants] = {};
    for (int32_t i = 0; i < B; ++i) {
      const int v = variant[static_cast<size_t>(i)];
      if (v < 0) continue;
      sfw_batch_rec *const rec = reinterpret_cast<sfw_batch_rec *>(pt + rec_at[v]) + filled[v];
      sfw_cycle_batch_record(L[static_cast<size_t>(i)], rec);
      reinterpret_cast<uint32_t *>(pt + first_at[v])[filled[v]] = blocks[v];
      blocks[v] += static_cast<uint32_t>(rec->L.chunk_count);
      lds[v] = std::max(lds[v], static_cast<size_t>(rec->lds_bytes));
      ++filled[v];
    }
    for (int v = 0; v < kVariants; ++v)
      if (count[v] > 0) reinterpret_cast<uint32_t *>(pt + first_at[v])[count[v]] = blocks[v];
    if (!(reuse_table && b->table.p && b->table_sent == b->table_host)) {
      b->table_sent.clear();  // (nothing is known of the device copy until the upload below is enqueued)
      if (b->pin_table.reserve(bytes) != hipSuccess || b->table.reserve(bytes) != hipSuccess)
        return bfail(b, SFW_ERR_HIP, "batch_launch: member table allocation failed");
      std::memcpy(b->pin_table.p, pt, bytes);
      if (hipMemcpyAsync(b->table.p, b->pin_table.p, bytes, hipMemcpyHostToDevice, b->stream) != hipSuccess ||
          b->pin_table.mark(b->stream) != hipSuccess)
        return bfail(b, SFW_ERR_HIP, "batch_launch: member table copy failed");
      b->table_sent.swap(b->table_host);
      ++b->table_uploads;
    }
    for (int v = 0; v < kVariants; ++v) {
      if (count[v] == 0) continue;
      const uint32_t *const d_first = reinterpret_cast<const uint32_t *>(b->table.p + first_at[v]);
      const sfw_batch_rec *const d_recs = reinterpret_cast<const sfw_batch_rec *>(b->table.p + rec_at[v]);
      const hipError_t e = v % 9 / 3 == 2 ? sfw_launch_cycle_batch_strict(v, d_first, d_recs, count[v], blocks[v], lds[v], b->stream)
                                      : sfw_launch_cycle_batch(v, d_first, d_recs, count[v], blocks[v], lds[v], b->stream);
      if (e != hipSuccess) return bfail(b, SFW_ERR_HIP, std::string("batch_launch: sfw_batch_cycle_kernel: ") + hipGetErrorString(e));
      ++d.batch_launches;
      d.batch_blocks += blocks[v];
      d.lds_bytes = std::max(d.lds_bytes, static_cast<int32_t>(lds[v]));
    }
    for (int32_t i = 0; i < B; ++i)
      if (variant[static_cast<size_t>(i)] >= 0 && cycle_commit(b->h[static_cast<size_t>(i)], false) != SFW_OK)
        return bmember_fail(b, i, SFW_ERR_HIP, "batch_launch");
  }
  // the others on their usual path, behind the batch launches on the same stream
  // (a list member's own path is what sfw_grid_launch would do: its own one-kernel cycle where that applies)
  for (int32_t i = 0; i < B; ++i) {
    const size_t m = static_cast<size_t>(i);
    if (variant[m] >= 0) continue;
    if (b->h[m]->st.list && cycle_launch_of(b->h[m], lp[m], L[m])) {
      if (const hipError_t e = launch_cycle_of(L[m], b->h[m]->stream); e != hipSuccess) {
        (void)hip_fail(b->h[m], e, "sfw_cycle_list_kernel");
        return bmember_fail(b, i, SFW_ERR_HIP, "batch_launch");
      }
      if (cycle_commit(b->h[m], false) != SFW_OK) return bmember_fail(b, i, SFW_ERR_HIP, "batch_launch");
      continue;
    }
    if (int e = launch_kernels(b->h[m], lp[m])) return bmember_fail(b, i, e, "batch_launch");
  }
  b->desc = d;
  b->launched = true;
  return SFW_OK;
}

int batch_launch(sfw_batch b, bool reuse_table = false) {
  // every member staged, or nothing is enqueued
  for (size_t i = 0; i < b->h.size(); ++i)
    if (!b->h[i]->st.valid)
      return bfail(b, SFW_ERR_STATE, "batch_launch: member " + std::to_string(i) + " has no staged grid (sfw_grid_stage; sfw_score_one consumes it)");
  const int rc = batch_enqueue(b, reuse_table);
  if (rc != SFW_OK)
    for (sfw_handle h : b->h) drop_launch(h);  // all or none: the members committed before the failure included
  return rc;
}

int batch_fetch(sfw_batch b, sfw_best *best_out) {
  const int32_t B = static_cast<int32_t>(b->h.size());
  for (int32_t i = 0; i < B; ++i)
    if (!b->h[static_cast<size_t>(i)]->last.launched)
      return bfail(b, SFW_ERR_STATE, "batch_fetch: member " + std::to_string(i) + " has not been launched");
  if (hipSetDevice(b->device) != hipSuccess) return bfail(b, SFW_ERR_HIP, "batch_fetch: hipSetDevice failed");
  // one wait for the whole batch (one stream)
  if (const hipError_t e = wait_stream(b->h[0]); e != hipSuccess) return bfail(b, SFW_ERR_HIP, std::string("batch_fetch: ") + hipGetErrorString(e));
  for (int32_t i = 0; i < B; ++i) {
    sfw_handle h = b->h[static_cast<size_t>(i)];
    stream_is_idle(h);
    sfw_best *const best = best_out ? best_out + i : nullptr;
    if (h->last.mirrored) {  // (as sfw_grid_fetch: the selection kernels left vector and record in the pinned mirror)
      h->last.fetched = true;
      sfw_sel s;
      std::memcpy(&s, h->pin_mirror.p + sizeof(double) * static_cast<size_t>(h->st.nv) * h->st.nw, sizeof(s));
      if (int e = sel_to_best(h, s, best, nullptr)) return bmember_fail(b, i, e, "batch_fetch");
    } else if (int e = sfw_grid_fetch(h, nullptr, best, nullptr)) {  // (a grid too large for the mirror: its own copy)
      return bmember_fail(b, i, e, "batch_fetch");
    }
  }
  return SFW_OK;
}

// The three list forms of sfw_batch_score_grid: every member's arguments are read against the single stage's rules before ANY
// member is staged (a refused call changes nothing), then stage (the member's own stage function, index_base 0), launch, fetch.
// `refusal(i)`: null, or why member i's arguments are refused; `stage(i)`: the member's stage call.
template <typename Refusal, typename Stage>
int batch_score_lists(sfw_batch b, const char *what, const char *common, Refusal refusal, Stage stage, sfw_best *best_out) {
  if (common) return bfail(b, SFW_ERR_INVALID_ARG, std::string(what) + ": " + common);
  for (size_t i = 0; i < b->h.size(); ++i)
    if (const char *why = refusal(i)) return bfail(b, SFW_ERR_INVALID_ARG, std::string(what) + " (member " + std::to_string(i) + "): " + why);
  const auto t0 = std::chrono::steady_clock::now();
  for (size_t i = 0; i < b->h.size(); ++i)
    if (int e = stage(i)) return bmember_fail(b, static_cast<int32_t>(i), e, (std::string(what) + ": stage").c_str());
  b->us[0] = us_since(t0);
  if (int e = sfw_batch_launch(b)) return e;
  return sfw_batch_fetch(b, best_out);
}
}  // namespace

extern "C" {

int sfw_batch_create(const sfw_params *params, int device, int32_t B, sfw_batch *out) {
  if (!out) return SFW_ERR_INVALID_ARG;
  *out = nullptr;
  if (B < 1 || B > SFW_BATCH_MAX) return SFW_ERR_INVALID_ARG;
  if (int e = check_params(nullptr, params)) return e;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return SFW_ERR_NO_DEVICE;
  if (device < 0 || device >= count) return SFW_ERR_INVALID_ARG;
  sfw_batch b = new (std::nothrow) sfw_batch_s();
  if (!b) return SFW_ERR_HIP;
  b->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&b->side, hipStreamNonBlocking);
  int rc = e == hipSuccess ? SFW_OK : SFW_ERR_HIP;
  for (int32_t i = 0; i < B && rc == SFW_OK; ++i) {
    sfw_handle h = nullptr;
    rc = create_handle(params, device, b->stream, b->side, &h);
    if (rc == SFW_OK) {
      h->cfg.batch_member = true;
      b->h.push_back(h);
    }
  }
  if (rc != SFW_OK) {
    sfw_batch_destroy(b);
    return rc;
  }
  *out = b;
  return SFW_OK;
}

int sfw_batch_destroy(sfw_batch b) {
  if (!b) return SFW_OK;
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  for (sfw_handle h : b->h) (void)destroy_handle(h);
  b->pin_table.release();
  b->table.release();
  if (b->side) (void)hipStreamDestroy(b->side);
  if (b->stream) (void)hipStreamDestroy(b->stream);
  delete b;
  return SFW_OK;
}

const char *sfw_batch_last_error(sfw_batch b) { return b ? b->err.c_str() : "null batch"; }

int32_t sfw_batch_size(sfw_batch b) { return b ? static_cast<int32_t>(b->h.size()) : 0; }

sfw_handle sfw_batch_member(sfw_batch b, int32_t i) {
  return (b && i >= 0 && i < static_cast<int32_t>(b->h.size())) ? b->h[static_cast<size_t>(i)] : nullptr;
}

int sfw_batch_launch(sfw_batch b) {
  if (!b) return SFW_ERR_INVALID_ARG;
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = batch_launch(b);
  b->us[1] = us_since(t0);
  return rc;
}

int sfw_batch_fetch(sfw_batch b, sfw_best *best_out) {
  if (!b) return SFW_ERR_INVALID_ARG;
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = batch_fetch(b, best_out);
  b->us[2] = us_since(t0);
  return rc;
}

int sfw_batch_score_grid(sfw_batch b, const sfw_robot_state *rs, const double *linvels, int32_t nv, const double *angvels,
                         int32_t nw, const sfw_goal_args *args, sfw_best *best_out) {
  if (!b) return SFW_ERR_INVALID_ARG;
  if (!rs || !args) return bfail(b, SFW_ERR_INVALID_ARG, "batch_score_grid: null robot states or goal arguments");
  const auto t0 = std::chrono::steady_clock::now();
  for (size_t i = 0; i < b->h.size(); ++i)
    if (int e = sfw_grid_stage(b->h[i], rs + i, linvels, nv, angvels, nw, args + i, 0))
      return bmember_fail(b, static_cast<int32_t>(i), e, "batch_score_grid: stage");
  b->us[0] = us_since(t0);
  if (int e = sfw_batch_launch(b)) return e;
  return sfw_batch_fetch(b, best_out);
}

int sfw_batch_set_list_fusion(sfw_batch b, int32_t enabled) {
  if (!b) return SFW_ERR_INVALID_ARG;
  b->list_fusion = enabled != 0;
  return SFW_OK;
}

int sfw_batch_get_list_fusion(sfw_batch b, int32_t *enabled_out) {
  if (!b || !enabled_out) return SFW_ERR_INVALID_ARG;
  *enabled_out = b->list_fusion ? 1 : 0;
  return SFW_OK;
}

int sfw_batch_score_samples(sfw_batch b, const sfw_robot_state *rs, const double *vx, const double *vy, const double *vtheta, int32_t n,
                            const sfw_goal_args *args, sfw_best *best_out) {
  if (!b) return SFW_ERR_INVALID_ARG;
  const char *const common = !rs || !args || !vx || !vtheta ? "null robot states, goal arguments or sample vectors" : n < 1 ? "n < 1" : nullptr;
  const size_t row = n > 0 ? static_cast<size_t>(n) : 0;
  const auto vy_of = [&](size_t i) { return vy ? vy + i * row : nullptr; };
  return batch_score_lists(
      b, "batch_score_samples", common,
      [&](size_t i) { return list_stage_refusal(rs + i, args + i, list_request(vx + i * row, vy_of(i), vtheta + i * row, n, 0)); },
      [&](size_t i) { return sfw_samples_stage(b->h[i], rs + i, vx + i * row, vy_of(i), vtheta + i * row, n, args + i, 0); }, best_out);
}

int sfw_batch_score_sequences(sfw_batch b, const sfw_robot_state *rs, const double *vx, const double *vy, const double *vtheta, int32_t n,
                              int32_t K, const int32_t *knot_step, const sfw_goal_args *args, sfw_best *best_out) {
  if (!b) return SFW_ERR_INVALID_ARG;
  const char *common = !rs || !args || !vx || !vtheta ? "null robot states, goal arguments or sample vectors" : n < 1 ? "n < 1" : nullptr;
  if (!common) common = sequences_refusal(K, knot_step);
  const size_t rows = common ? 0 : static_cast<size_t>(K) * static_cast<size_t>(n);
  const auto vy_of = [&](size_t i) { return vy ? vy + i * rows : nullptr; };
  return batch_score_lists(
      b, "batch_score_sequences", common,
      [&](size_t i) {
        return list_stage_refusal(rs + i, args + i, sequences_request(vx + i * rows, vy_of(i), vtheta + i * rows, n, K, knot_step, 0));
      },
      [&](size_t i) {
        return sfw_sequences_stage(b->h[i], rs + i, vx + i * rows, vy_of(i), vtheta + i * rows, n, K, knot_step, args + i, 0);
      },
      best_out);
}

int sfw_batch_score_perturbed(sfw_batch b, const sfw_robot_state *rs, const sfw_perturb *p, int32_t n, int32_t K,
                              const int32_t *knot_step, const sfw_goal_args *args, sfw_best *best_out) {
  if (!b) return SFW_ERR_INVALID_ARG;
  const char *const common = !rs || !args || !p ? "null robot states, goal arguments or perturbations" : nullptr;
  return batch_score_lists(
      b, "batch_score_perturbed", common,
      [&](size_t i) {
        if (const char *why = perturb_refusal(rs + i, p + i, n, K, knot_step, args + i, 0)) return why;
        return list_stage_refusal(rs + i, args + i, perturbed_request(nullptr, n, K, knot_step, 0));
      },
      [&](size_t i) { return sfw_sequences_perturb_stage(b->h[i], rs + i, p + i, n, K, knot_step, args + i, 0); }, best_out);
}

int sfw_batch_describe(sfw_batch b, sfw_batch_desc *out) {
  if (!b || !out) return SFW_ERR_INVALID_ARG;
  if (!b->launched) return bfail(b, SFW_ERR_STATE, "batch_describe before batch_launch");
  *out = b->desc;
  return SFW_OK;
}

int sfw_batch_last_us(sfw_batch b, int32_t which, double *us_out) {
  if (!b || !us_out) return SFW_ERR_INVALID_ARG;
  if (which < 0 || which > 2) return bfail(b, SFW_ERR_INVALID_ARG, "batch_last_us: which must be 0..2");
  *us_out = b->us[which];
  return SFW_OK;
}

}  // extern "C"

// ===========================================================================
// one grid under several crowd hypotheses (sfw_ensemble_*)
// ===========================================================================
struct sfw_ensemble_s {
  int device = 0;
  sfw_params params;
  sfw_batch b = nullptr;       // the M members (terms capture on), one stream
  std::vector<char> hyp_set;   // sfw_ensemble_set_hypothesis(m) has been called
  std::string err;
  // pinned: the record | costs (T doubles) | rejected (T int32), written by the aggregation kernels; a grid whose cost vector
  // exceeds the members' mirror size (SFW_MIRROR_MAX_MB) leaves costs | rejected in d_out instead (copied out after the wait)
  pinned_buf pin_out;
  pinned_buf pin_tab;          // M term-buffer pointers | M probabilities: ONE H2D per aggregation, guarded by its event
  dev_buf<char> tab, d_out;
  dev_buf<sfw_sel> partials;
  bool scored = false;         // a score_grid completed; seq: every member's launch_seq at its end
  bool mirrored = false;       // the last aggregation wrote costs | rejected to pin_out
  std::vector<uint64_t> seq;
  int64_t T = 0;
  double us[3] = {0.0, 0.0, 0.0};
  // sfw_ensemble_blend: the last aggregation's cost vector ON THE DEVICE — d_out when it went there, d_cost when it went to
  // the pinned mirror (a list's aggregation writes both; a grid's is uploaded by the first blend that asks: cost_dev null) —
  // and the blend's own buffers (member 0's belong to its sfw_grid_blend)
  dev_buf<double> d_cost;
  const double *cost_dev = nullptr;
  blend_buffers blend;
  // sfw_ensemble_blend_control: the control cost's bias vector (member 0's ctrl_bias belongs to its sfw_grid_blend_control).
  // sfw_ensemble_mppi_run: the chain's buffers, and the members' knot rows as sfw_perturb_members_kernel reads them (M
  // sfw_perturb_dst: the table behind the nominal in pin_mppi is the source of its copy)
  mppi_buffers mppi;
  dev_buf<sfw_perturb_dst> pert_dst;
  // sfw_ensemble_set_risk: read by every aggregation while risk_on (ensemble_check_mode, ensemble_enqueue)
  sfw_risk risk{1.0, 0.0, 0};
  bool risk_on = false;
  int64_t chain_uploads = 0;  // member-table uploads of the last sfw_ensemble_mppi_run's batched launches (sfw_ensemble_batch_desc)
};

namespace {
constexpr size_t kEnsRecBytes = (sizeof(sfw_sel) + 15) & ~size_t(15);

int efail(sfw_ensemble e, int code, const std::string &msg) {
  if (e) e->err = msg;
  return code;
}
int emember_fail(sfw_ensemble e, int32_t m, int code, const char *what) {
  return efail(e, code, std::string(what) + " (member " + std::to_string(m) + "): " + e->b->h[static_cast<size_t>(m)]->err);
}
// f(member) for every member in order, until one fails: that member's failure under `what`
template <typename F>
int ensemble_each(sfw_ensemble e, const char *what, F f) {
  for (size_t m = 0; m < e->b->h.size(); ++m)
    if (int rc = f(e->b->h[m])) return emember_fail(e, static_cast<int32_t>(m), rc, what);
  return SFW_OK;
}
// P of the risk's definition: ((0.0 + p[0]) + p[1]) + ... in member order, p[m] = 1.0 / M without probabilities
double ensemble_mass(int32_t M, const double *probs) {
  double P = 0.0;
  for (int32_t m = 0; m < M; ++m) P = P + (probs ? probs[m] : 1.0 / M);
  return P;
}
// mode and probabilities: no device call
int ensemble_check_mode(sfw_ensemble e, int32_t mode, const double *probs, const char *what) {
  if (mode != SFW_ENSEMBLE_MEAN && mode != SFW_ENSEMBLE_MAX)
    return efail(e, SFW_ERR_INVALID_ARG, std::string(what) + ": mode must be SFW_ENSEMBLE_MEAN or SFW_ENSEMBLE_MAX");
  if (probs)
    for (size_t m = 0; m < e->hyp_set.size(); ++m)
      if (!std::isfinite(probs[m]) || !(probs[m] >= 0.0))
        return efail(e, SFW_ERR_INVALID_ARG, std::string(what) + ": probability " + std::to_string(m) + " is not finite and >= 0");
  if (e->risk_on && ensemble_mass(static_cast<int32_t>(e->hyp_set.size()), probs) == 0.0)
    return efail(e, SFW_ERR_INVALID_ARG, std::string(what) + ": every probability is zero under a risk (sfw_ensemble_set_risk)");
  return SFW_OK;
}

// The aggregation behind the members' launch on the batch's stream: member table upload, stage 1 (+ stage 2), and for a grid
// too large for the mirror nothing more (ensemble_finish copies it out after the wait).  reuse_tab: the member table on the
// device is the last aggregation's and would be the same bytes (sfw_ensemble_mppi_run, iterations > 0: same members, same
// probabilities) — no reserve of the pinned table, which waits for the last upload, and no upload.
int ensemble_enqueue(sfw_ensemble e, int32_t mode, const double *probs, bool reuse_tab = false) {
  const int32_t M = static_cast<int32_t>(e->b->h.size());
  sfw_handle h0 = e->b->h[0];
  const int64_t T = static_cast<int64_t>(h0->st.nv) * h0->st.nw;
  const size_t cost_bytes = sizeof(double) * static_cast<size_t>(T);
  const size_t rej_bytes = (sizeof(int32_t) * static_cast<size_t>(T) + 15) & ~size_t(15);
  e->T = T;
  e->mirrored = cost_bytes <= h0->cfg.mirror_max_bytes;  // (the handle's rule: pinned up to SFW_MIRROR_MAX_MB of costs)
  const bool list = h0->st.list;  // the members staged sequences (a list): the list form of stage 1
  e->cost_dev = nullptr;
  if (e->pin_out.reserve(kEnsRecBytes + (e->mirrored ? cost_bytes + rej_bytes : 0)) != hipSuccess ||
      (!e->mirrored && e->d_out.reserve(cost_bytes + rej_bytes) != hipSuccess) ||
      (e->mirrored && list && e->d_cost.reserve(static_cast<size_t>(T)) != hipSuccess) ||
      e->partials.reserve(static_cast<size_t>(sfw_argmin_partials(T))) != hipSuccess)
    return efail(e, SFW_ERR_HIP, "ensemble: output allocation failed");
  const size_t tab_bytes = 2 * sizeof(double) * static_cast<size_t>(M);
  if (!reuse_tab) {
    if (e->pin_tab.reserve(tab_bytes) != hipSuccess || e->tab.reserve(tab_bytes) != hipSuccess)
      return efail(e, SFW_ERR_HIP, "ensemble: member table allocation failed");
    const double **ptrs = reinterpret_cast<const double **>(e->pin_tab.p);
    double *const p = reinterpret_cast<double *>(e->pin_tab.p + sizeof(double) * static_cast<size_t>(M));
    for (int32_t m = 0; m < M; ++m) {
      ptrs[m] = e->b->h[static_cast<size_t>(m)]->terms.p;
      p[m] = probs ? probs[m] : 1.0 / M;
    }
    if (hipMemcpyAsync(e->tab.p, e->pin_tab.p, tab_bytes, hipMemcpyHostToDevice, e->b->stream) != hipSuccess ||
        e->pin_tab.mark(e->b->stream) != hipSuccess)
      return efail(e, SFW_ERR_HIP, "ensemble: member table copy failed");
  }
  const sfw_weights w{e->params.vel_weight, e->params.distance_weight, e->params.angle_weight, e->params.costmap_weight,
                      e->params.social_weight};
  char *const out = e->mirrored ? e->pin_out.p + kEnsRecBytes : e->d_out.p;
  const double *const *const d_terms = reinterpret_cast<const double *const *>(e->tab.p);
  const double *const d_probs = reinterpret_cast<const double *>(e->tab.p + sizeof(double) * static_cast<size_t>(M));
  const double thr = e->risk_on ? e->risk.contact_mass * ensemble_mass(M, probs) : 0.0;  // (the risk's contact threshold: one product)
  // sfw_set_path: member 0's term and weight as its stage found them (null: the five terms alone)
  const double *const path_p = h0->st.path_on ? h0->path_p.p : nullptr;
  const double path_w = h0->st.path_weight;
  sfw_ensemble_launch a{};
  a.terms = d_terms;
  a.probs = d_probs;
  a.M = M;
  a.T = T;
  a.mode = mode;
  a.w = w;
  a.list = list;
  a.linvels = h0->st.d_linvels;
  a.angvels = h0->st.d_angvels;
  a.nw = h0->st.nw;
  a.costs = reinterpret_cast<double *>(out);
  a.costs_dev = list && e->mirrored ? e->d_cost.p : nullptr;
  a.rejected = reinterpret_cast<int32_t *>(out + cost_bytes);
  a.partials = e->partials.p;
  a.sel_host = reinterpret_cast<sfw_sel *>(e->pin_out.p);
  a.risk = e->risk_on;
  a.tail_mass = e->risk.tail_mass;
  a.contact_mass = e->risk.contact_mass;
  a.thr = thr;
  a.path_p = path_p;
  a.path_w = path_w;
  const hipError_t he = sfw_launch_ensemble(a, e->b->stream);
  if (he != hipSuccess)
    return efail(e, SFW_ERR_HIP, std::string(e->risk_on ? (list ? "ensemble: sfw_ens_risk_list / sfw_ensemble_stage2: "
                                                                : "ensemble: sfw_ens_risk_grid / sfw_ensemble_stage2: ")
                                             : list   ? "ensemble: sfw_ens_list_first / sfw_ensemble_stage2: "
                                                      : "ensemble: sfw_ensemble_stage1/2: ") +
                                     hipGetErrorString(he));
  e->cost_dev = !e->mirrored ? reinterpret_cast<const double *>(e->d_out.p) : list ? e->d_cost.p : nullptr;
  return SFW_OK;
}

// After the wait: the outputs to the caller
int ensemble_finish(sfw_ensemble e, double *costs_out, int32_t *rejected_out, sfw_best *best_out) {
  e->pin_tab.pending = false;
  const size_t cost_bytes = sizeof(double) * static_cast<size_t>(e->T), rej_bytes = sizeof(int32_t) * static_cast<size_t>(e->T);
  if (e->mirrored) {
    if (costs_out) std::memcpy(costs_out, e->pin_out.p + kEnsRecBytes, cost_bytes);
    if (rejected_out) std::memcpy(rejected_out, e->pin_out.p + kEnsRecBytes + cost_bytes, rej_bytes);
  } else {
    if (costs_out && hipMemcpy(costs_out, e->d_out.p, cost_bytes, hipMemcpyDeviceToHost) != hipSuccess)
      return efail(e, SFW_ERR_HIP, "ensemble: cost copy failed");
    if (rejected_out && hipMemcpy(rejected_out, e->d_out.p + cost_bytes, rej_bytes, hipMemcpyDeviceToHost) != hipSuccess)
      return efail(e, SFW_ERR_HIP, "ensemble: rejected copy failed");
  }
  sfw_sel s;
  std::memcpy(&s, e->pin_out.p, sizeof(s));
  // (member 0 holds what the record refers to: a grid's axes, a list's first knot row — on the device after a perturbed stage)
  if (int rc = sel_to_best(e->b->h[0], s, best_out, nullptr)) return emember_fail(e, 0, rc, "ensemble: winner's first knot");
  return SFW_OK;
}

// The state rules every ensemble score shares, after the arguments and before any member is staged
int ensemble_check_members(sfw_ensemble e, const char *what) {
  for (size_t m = 0; m < e->b->h.size(); ++m) {
    const sfw_handle h = e->b->h[m];
    if (!e->hyp_set[m]) return efail(e, SFW_ERR_STATE, std::string(what) + ": hypothesis " + std::to_string(m) + " was never set");
    if (std::memcmp(&h->live.params, &e->params, sizeof(sfw_params)) != 0)
      return efail(e, SFW_ERR_STATE, std::string(what) + ": member " + std::to_string(m) + "'s sfw_params differ from the ensemble's");
    if (!h->live.capture_terms)
      return efail(e, SFW_ERR_STATE, std::string(what) + ": member " + std::to_string(m) + "'s terms capture was turned off");
    if (!h->world.have_costmap) return efail(e, SFW_ERR_STATE, std::string(what) + ": no costmap set (sfw_ensemble_set_costmap)");
    // the aggregation adds member 0's path term: every member must have the same path, bit for bit (sfw_ensemble_set_path)
    const sfw_handle h0 = e->b->h[0];
    if (h->live.path_on != h0->live.path_on || std::memcmp(&h->live.path_weight, &h0->live.path_weight, sizeof(double)) != 0 ||
        h->live.path_xy.size() != h0->live.path_xy.size() ||
        (!h->live.path_xy.empty() && std::memcmp(h->live.path_xy.data(), h0->live.path_xy.data(), sizeof(double) * h->live.path_xy.size()) != 0))
      return efail(e, SFW_ERR_STATE, std::string(what) + ": member " + std::to_string(m) + "'s path differs from member 0's (sfw_ensemble_set_path)");
  }
  return SFW_OK;
}

// The state rule of sfw_ensemble_aggregate and sfw_ensemble_blend: something was scored, and no member has moved since
int ensemble_check_scored(sfw_ensemble e, const char *what) {
  if (!e->scored) return efail(e, SFW_ERR_STATE, std::string(what) + ": nothing scored (sfw_ensemble_score_grid / _sequences / _perturbed)");
  for (size_t m = 0; m < e->b->h.size(); ++m) {
    const sfw_handle h = e->b->h[m];
    if (!h->last.launched || !h->last.terms || h->launch_seq != e->seq[m])
      return efail(e, SFW_ERR_STATE, std::string(what) + ": member " + std::to_string(m) +
                                         " was staged, launched or used for sfw_score_one since the last score");
  }
  return SFW_OK;
}

// How every ensemble score begins: the mode, the stage's argument rules (`why`: null, or what they refuse — read before ANY member
// is staged, so that a refused call leaves the previous score as it was), the members' state; then nothing is scored any more
int ensemble_score_begin(sfw_ensemble e, const char *what, int32_t mode, const double *probs, const std::string &why) {
  if (!e) return SFW_ERR_INVALID_ARG;
  if (int rc = ensemble_check_mode(e, mode, probs, what)) return rc;
  if (!why.empty()) return efail(e, SFW_ERR_INVALID_ARG, std::string(what) + ": " + why);
  if (int rc = ensemble_check_members(e, what)) return rc;
  e->scored = false;
  if (hipSetDevice(e->device) != hipSuccess) return efail(e, SFW_ERR_HIP, std::string(what) + ": hipSetDevice failed");
  return SFW_OK;
}
// A whole ensemble score (the shape of sfw_ensemble_score_grid): that beginning, the timed loop that stages every member, one batch
// launch, the aggregation behind it, one wait
template <typename Stage>
int ensemble_score(sfw_ensemble e, const std::string &what, int32_t mode, const double *probs, const char *why, Stage stage,
                   double *costs_out, int32_t *rejected_out, sfw_best *best_out) {
  if (int rc = ensemble_score_begin(e, what.c_str(), mode, probs, why ? why : "")) return rc;
  const size_t M = e->b->h.size();
  auto t0 = std::chrono::steady_clock::now();
  if (int rc = ensemble_each(e, (what + ": stage").c_str(), stage)) return rc;
  e->us[0] = us_since(t0);
  t0 = std::chrono::steady_clock::now();
  if (int rc = batch_launch(e->b)) return efail(e, rc, what + ": " + e->b->err);
  for (size_t m = 0; m < M; ++m)
    if (!e->b->h[m]->last.terms) return efail(e, SFW_ERR_STATE, what + ": member " + std::to_string(m) + " did not capture terms");
  if (int rc = ensemble_enqueue(e, mode, probs)) return rc;
  e->us[1] = us_since(t0);
  t0 = std::chrono::steady_clock::now();
  if (int rc = batch_fetch(e->b, nullptr)) return efail(e, rc, what + ": " + e->b->err);  // (one wait, all members)
  if (int rc = ensemble_finish(e, costs_out, rejected_out, best_out)) return rc;
  e->us[2] = us_since(t0);
  for (size_t m = 0; m < M; ++m) e->seq[m] = e->b->h[m]->launch_seq;
  e->scored = true;
  return SFW_OK;
}

// sfw_ensemble_blend (gamma null) and sfw_ensemble_blend_control over the last aggregation's cost vector: ONE text.  The control
// cost is that of member 0's perturbed stage (every member staged the same sfw_perturb), into the ensemble's own bias buffer.
int ensemble_blend(sfw_ensemble e, const char *what, const double *lambda, int32_t L, const double *gamma, const double *bias,
                   sfw_blend_stat *stat_out, double *u_out, double *weights_out) {
  if (!e) return SFW_ERR_INVALID_ARG;
  if (const char *why = blend_refusal(lambda, L, stat_out, u_out)) return efail(e, SFW_ERR_INVALID_ARG, std::string(what) + ": " + why);
  if (gamma && !std::isfinite(*gamma)) return efail(e, SFW_ERR_INVALID_ARG, std::string(what) + ": gamma is not finite");
  if (int rc = ensemble_check_scored(e, what)) return rc;
  sfw_handle h0 = e->b->h[0];
  if (gamma)
    if (const char *why = control_state_refusal(h0))
      return efail(e, SFW_ERR_STATE, std::string(what) + ": the last score was not a perturbed one: " + why);
  if (bias && !all_finite(bias, static_cast<size_t>(e->T))) return efail(e, SFW_ERR_INVALID_ARG, std::string(what) + ": non-finite bias");
  if (hipSetDevice(e->device) != hipSuccess) return efail(e, SFW_ERR_HIP, std::string(what) + ": hipSetDevice failed");
  if (!e->cost_dev) {  // a grid's aggregation left the vector in the pinned mirror only: the blend's kernels read a device copy
    if (!e->mirrored) return efail(e, SFW_ERR_STATE, std::string(what) + ": the last aggregation left no cost vector");
    if (e->d_cost.reserve(static_cast<size_t>(e->T)) != hipSuccess ||
        hipMemcpyAsync(e->d_cost.p, e->pin_out.p + kEnsRecBytes, sizeof(double) * static_cast<size_t>(e->T), hipMemcpyHostToDevice,
                       e->b->stream) != hipSuccess)
      return efail(e, SFW_ERR_HIP, std::string(what) + ": cost vector upload failed");
    e->cost_dev = e->d_cost.p;  // (the blend waits for the stream before it returns: the mirror is free again by then)
  }
  // gamma == 0: the plain blend (as sfw_grid_blend_control)
  const double *d_bias = nullptr;
  if (gamma && *gamma != 0.0) {
    if (int rc = control_cost_enqueue(h0, *gamma, bias, nullptr, e->mppi, e->blend)) return emember_fail(e, 0, rc, what);
    d_bias = e->mppi.ctrl_bias.p;
    bias = nullptr;
  }
  if (int rc = blend_run(h0, e->blend, e->cost_dev, e->T, lambda, L, bias, stat_out, u_out, weights_out, d_bias))
    return emember_fail(e, 0, rc, what);
  return SFW_OK;
}

// sfw_ensemble_mppi_run behind its stage of iteration 0: everything enqueued on the batch's stream, one wait, the outputs.  A
// failure is the caller's to clean up.  The members are lists: without list fusion batch_launch builds no member table (each
// takes its own path); with it (sfw_ensemble_set_list_fusion) every iteration is one batched launch, whose member table an
// iteration > 0 reads again from the device when its records are the bytes last uploaded (batch_enqueue reuse_table).  The
// aggregation's table is uploaded by iteration 0 and read again from the device by the others.
int ensemble_mppi_chain(sfw_ensemble e, const sfw_perturb *p, int32_t mode, const double *probs, const sfw_mppi *m,
                        sfw_blend_stat *stat_out, double *plans_out, double *costs_out, int32_t *rejected_out, sfw_best *best_out) {
  const char *const what = "ensemble_mppi_run";
  const size_t M = e->b->h.size();
  sfw_handle h0 = e->b->h[0];
  const int I = m->iterations, K = h0->st.nk;
  const int64_t n = h0->st.nv;
  const size_t dst_bytes = sizeof(sfw_perturb_dst) * M;
  const mppi_slots s(I, K, dst_bytes);
  if (s.bytes > e->mppi.pin_mppi.cap && hipStreamSynchronize(e->b->stream) != hipSuccess)
    return efail(e, SFW_ERR_HIP, std::string(what) + ": hipStreamSynchronize failed");
  if (mppi_reserve(e->mppi, e->blend, s, K, n, m->gamma != 0.0) != hipSuccess || e->pert_dst.reserve(M) != hipSuccess ||
      e->d_cost.reserve(static_cast<size_t>(n)) != hipSuccess)
    return efail(e, SFW_ERR_HIP, std::string(what) + ": allocation failed");
  char *const pin = e->mppi.pin_mppi.p;
  std::memcpy(pin + s.plan_at, p->nominal, s.plan_bytes);
  sfw_perturb_dst *const dst = reinterpret_cast<sfw_perturb_dst *>(pin + s.extra_at);
  for (size_t k = 0; k < M; ++k) {
    const sfw_handle h = e->b->h[k];
    dst[k] = sfw_perturb_dst{const_cast<double *>(h->st.d_linvels), const_cast<double *>(h->st.d_vy), const_cast<double *>(h->st.d_angvels),
                             h->st.normals_kept ? h->normals.p : nullptr};
  }
  if (hipMemcpyAsync(e->mppi.mppi_plan.p, pin + s.plan_at, s.plan_bytes, hipMemcpyHostToDevice, e->b->stream) != hipSuccess ||
      hipMemcpyAsync(e->pert_dst.p, dst, dst_bytes, hipMemcpyHostToDevice, e->b->stream) != hipSuccess)
    return efail(e, SFW_ERR_HIP, std::string(what) + ": plan or member table copy failed");
  double *const plan = e->mppi.mppi_plan.p;
  auto t0 = std::chrono::steady_clock::now();
  const int64_t uploads0 = e->b->table_uploads;
  for (int i = 0; i < I; ++i) {
    if (i > 0) {  // the stage of iteration i: its seed, and every member's knots drawn once around the plan the last update left
      for (sfw_handle h : e->b->h) perturb_seed(h->st.pert, p->seed + static_cast<uint64_t>(i));
      if (const hipError_t he = sfw_launch_perturb_members(h0->st.pert, plan, n, K, 0, e->pert_dst.p, static_cast<int>(M), e->b->stream);
          he != hipSuccess)
        return efail(e, SFW_ERR_HIP, std::string(what) + ": sfw_perturb_members_kernel: " + hipGetErrorString(he));
    }
    if (int rc = batch_launch(e->b, i > 0)) return efail(e, rc, std::string(what) + ": " + e->b->err);
    for (size_t k = 0; k < M; ++k)
      if (!e->b->h[k]->last.terms) return efail(e, SFW_ERR_STATE, std::string(what) + ": member " + std::to_string(k) + " did not capture terms");
    if (int rc = ensemble_enqueue(e, mode, probs, i > 0)) return rc;
    const double *d_bias = nullptr;
    if (m->gamma != 0.0) {  // (as sfw_ensemble_blend_control: gamma == 0 is the plain blend)
      if (int rc = control_cost_enqueue(h0, m->gamma, nullptr, plan, e->mppi, e->blend)) return emember_fail(e, 0, rc, what);
      d_bias = e->mppi.ctrl_bias.p;
    }
    if (int rc = blend_enqueue(h0, e->blend, e->cost_dev, n, &m->lambda, 1, d_bias, nullptr, pin + i * s.slot, plan))
      return emember_fail(e, 0, rc, what);
  }
  if (e->mppi.pin_mppi.mark(e->b->stream) != hipSuccess) return efail(e, SFW_ERR_HIP, std::string(what) + ": hipEventRecord failed");
  e->chain_uploads = e->b->table_uploads - uploads0;
  e->us[1] = us_since(t0);
  t0 = std::chrono::steady_clock::now();
  if (int rc = batch_fetch(e->b, nullptr)) return efail(e, rc, std::string(what) + ": " + e->b->err);  // THE wait, all members
  e->mppi.pin_mppi.pending = false;
  if (int rc = ensemble_finish(e, costs_out, rejected_out, best_out)) return rc;
  mppi_finish(s, pin, m, K, stat_out, plans_out, e->b->h.data(), M);
  e->us[2] = us_since(t0);
  for (size_t k = 0; k < M; ++k) e->seq[k] = e->b->h[k]->launch_seq;
  e->scored = true;
  return SFW_OK;
}
}  // namespace

extern "C" {

int sfw_ensemble_create(const sfw_params *params, int device, int32_t M, sfw_ensemble *out) {
  if (!out) return SFW_ERR_INVALID_ARG;
  *out = nullptr;
  if (M < 1 || M > SFW_ENSEMBLE_MAX_M) return SFW_ERR_INVALID_ARG;
  if (int rc = check_params(nullptr, params)) return rc;
  sfw_batch b = nullptr;
  if (int rc = sfw_batch_create(params, device, M, &b)) return rc;
  sfw_ensemble e = new (std::nothrow) sfw_ensemble_s();
  if (!e) {
    sfw_batch_destroy(b);
    return SFW_ERR_HIP;
  }
  e->device = device;
  e->params = *params;
  e->b = b;
  e->hyp_set.assign(static_cast<size_t>(M), 0);
  e->seq.assign(static_cast<size_t>(M), 0);
  for (sfw_handle h : b->h) h->live.capture_terms = true;
  *out = e;
  return SFW_OK;
}

int sfw_ensemble_destroy(sfw_ensemble e) {
  if (!e) return SFW_OK;
  (void)hipSetDevice(e->device);
  sfw_batch_destroy(e->b);  // (waits for the stream)
  e->pin_out.release();
  e->pin_tab.release();
  e->tab.release();
  e->d_out.release();
  e->partials.release();
  e->d_cost.release();
  e->blend.release();
  e->mppi.release();
  e->pert_dst.release();
  delete e;
  return SFW_OK;
}

const char *sfw_ensemble_last_error(sfw_ensemble e) { return e ? e->err.c_str() : "null ensemble"; }

int32_t sfw_ensemble_size(sfw_ensemble e) { return e ? static_cast<int32_t>(e->b->h.size()) : 0; }

sfw_handle sfw_ensemble_member(sfw_ensemble e, int32_t m) { return e ? sfw_batch_member(e->b, m) : nullptr; }

int sfw_ensemble_set_params(sfw_ensemble e, const sfw_params *params) {
  if (!e) return SFW_ERR_INVALID_ARG;
  if (int rc = check_params(nullptr, params)) return efail(e, rc, "ensemble_set_params: invalid parameters");
  if (int rc = ensemble_each(e, "ensemble_set_params", [&](sfw_handle h) { return sfw_set_params(h, params); })) return rc;
  e->params = *params;
  return SFW_OK;
}

int sfw_ensemble_set_costmap(sfw_ensemble e, const uint8_t *cells, uint32_t size_x, uint32_t size_y, double origin_x,
                             double origin_y, double resolution) {
  if (!e) return SFW_ERR_INVALID_ARG;
  return ensemble_each(e, "ensemble_set_costmap",
                       [&](sfw_handle h) { return sfw_set_costmap(h, cells, size_x, size_y, origin_x, origin_y, resolution); });
}

int sfw_ensemble_set_footprint(sfw_ensemble e, const double *xy, int32_t K) {
  if (!e) return SFW_ERR_INVALID_ARG;
  return ensemble_each(e, "ensemble_set_footprint", [&](sfw_handle h) { return sfw_set_footprint(h, xy, K); });
}

int sfw_ensemble_set_stop_check(sfw_ensemble e, const sfw_stop_check *c) {
  if (!e) return SFW_ERR_INVALID_ARG;
  // (the checks are the same for every member: the first one refuses before any member has changed)
  return ensemble_each(e, "ensemble_set_stop_check", [&](sfw_handle h) { return sfw_set_stop_check(h, c); });
}

int sfw_ensemble_set_path(sfw_ensemble e, const sfw_path *p) {
  if (!e) return SFW_ERR_INVALID_ARG;
  // (the checks are the same for every member: the first one refuses before any member has changed)
  return ensemble_each(e, "ensemble_set_path", [&](sfw_handle h) { return sfw_set_path(h, p); });
}

int sfw_ensemble_set_hypothesis(sfw_ensemble e, int32_t m, const sfw_agent *agents, int32_t A, const double *obstacles_xy,
                                int32_t O) {
  if (!e) return SFW_ERR_INVALID_ARG;
  if (m < 0 || m >= static_cast<int32_t>(e->b->h.size())) return efail(e, SFW_ERR_INVALID_ARG, "ensemble_set_hypothesis: m out of range");
  if (int rc = sfw_set_agents(e->b->h[static_cast<size_t>(m)], agents, A, obstacles_xy, O))
    return emember_fail(e, m, rc, "ensemble_set_hypothesis");
  e->hyp_set[static_cast<size_t>(m)] = 1;
  return SFW_OK;
}

int sfw_ensemble_score_grid(sfw_ensemble e, const sfw_robot_state *rs, const double *linvels, int32_t nv, const double *angvels,
                            int32_t nw, const sfw_goal_args *args, int32_t mode, const double *probs, double *costs_out,
                            int32_t *rejected_out, sfw_best *best_out) {
  const char *const why =
      !rs || !args || !linvels || !angvels || nv <= 0 || nw <= 0 ? "null robot state, goal arguments or sample vectors" : nullptr;
  return ensemble_score(
      e, "ensemble_score_grid", mode, probs, why, [&](sfw_handle h) { return sfw_grid_stage(h, rs, linvels, nv, angvels, nw, args, 0); },
      costs_out, rejected_out, best_out);
}

int sfw_ensemble_score_sequences(sfw_ensemble e, const sfw_robot_state *rs, const double *vx, const double *vy, const double *vtheta,
                                 int32_t n, int32_t K, const int32_t *knot_step, const sfw_goal_args *args, int32_t mode,
                                 const double *probs, double *costs_out, int32_t *rejected_out, sfw_best *best_out) {
  const char *why = sequences_refusal(K, knot_step);
  if (!why) why = list_stage_refusal(rs, args, sequences_request(vx, vy, vtheta, n, K, knot_step, 0));
  return ensemble_score(
      e, "ensemble_score_sequences", mode, probs, why,
      [&](sfw_handle h) { return sfw_sequences_stage(h, rs, vx, vy, vtheta, n, K, knot_step, args, 0); }, costs_out, rejected_out, best_out);
}

int sfw_ensemble_score_perturbed(sfw_ensemble e, const sfw_robot_state *rs, const sfw_perturb *p, int32_t n, int32_t K,
                                 const int32_t *knot_step, const sfw_goal_args *args, int32_t mode, const double *probs,
                                 double *costs_out, int32_t *rejected_out, sfw_best *best_out) {
  const char *why = perturb_refusal(rs, p, n, K, knot_step, args, 0);
  if (!why) why = list_stage_refusal(rs, args, perturbed_request(nullptr, n, K, knot_step, 0));
  // (every member draws the knots itself: a function of (seed, index, knot, channel) alone, so bitwise the same M times)
  return ensemble_score(
      e, "ensemble_score_perturbed", mode, probs, why,
      [&](sfw_handle h) { return sfw_sequences_perturb_stage(h, rs, p, n, K, knot_step, args, 0); }, costs_out, rejected_out, best_out);
}

int sfw_ensemble_blend(sfw_ensemble e, const double *lambda, int32_t L, const double *bias, sfw_blend_stat *stat_out, double *u_out,
                       double *weights_out) {
  return ensemble_blend(e, "ensemble_blend", lambda, L, nullptr, bias, stat_out, u_out, weights_out);
}

int sfw_ensemble_blend_control(sfw_ensemble e, const double *lambda, int32_t L, double gamma, const double *bias,
                               sfw_blend_stat *stat_out, double *u_out, double *weights_out) {
  return ensemble_blend(e, "ensemble_blend_control", lambda, L, &gamma, bias, stat_out, u_out, weights_out);
}

int sfw_ensemble_mppi_run(sfw_ensemble e, const sfw_robot_state *rs, const sfw_perturb *p, int32_t n, int32_t K, const int32_t *knot_step,
                          const sfw_goal_args *args, int32_t mode, const double *probs, const sfw_mppi *m, sfw_blend_stat *stat_out,
                          double *plans_out, double *costs_out, int32_t *rejected_out, sfw_best *best_out) {
  std::string why;
  if (const char *w = mppi_refusal(m)) why = std::string(w == kMppiIterations ? "m is NULL, " : "") + w;
  else if (!stat_out || !plans_out) why = "stat_out or plans_out is NULL";
  else if (const char *w = perturb_refusal(rs, p, n, K, knot_step, args, 0)) why = w;
  else if (const char *w = list_stage_refusal(rs, args, perturbed_request(nullptr, n, K, knot_step, 0))) why = w;
  if (int rc = ensemble_score_begin(e, "ensemble_mppi_run", mode, probs, why)) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  // iteration 0's stage: sfw_ensemble_score_perturbed's
  int rc = ensemble_each(e, "ensemble_mppi_run: stage",
                         [&](sfw_handle h) { return sfw_sequences_perturb_stage(h, rs, p, n, K, knot_step, args, 0); });
  e->us[0] = us_since(t0);
  if (rc == SFW_OK) rc = ensemble_mppi_chain(e, p, mode, probs, m, stat_out, plans_out, costs_out, rejected_out, best_out);
  if (rc != SFW_OK) {  // nothing scored, and no member left staged or launched
    if (e->mppi.pin_mppi.done) (void)e->mppi.pin_mppi.mark(e->b->stream);  // (kernels of the chain may still be writing there)
    for (sfw_handle h : e->b->h) drop_stage(h);
  }
  return rc;
}

int sfw_ensemble_aggregate(sfw_ensemble e, int32_t mode, const double *probs, double *costs_out, int32_t *rejected_out,
                           sfw_best *best_out) {
  if (!e) return SFW_ERR_INVALID_ARG;
  if (int rc = ensemble_check_mode(e, mode, probs, "ensemble_aggregate")) return rc;
  if (int rc = ensemble_check_scored(e, "ensemble_aggregate")) return rc;
  if (hipSetDevice(e->device) != hipSuccess) return efail(e, SFW_ERR_HIP, "ensemble_aggregate: hipSetDevice failed");
  auto t0 = std::chrono::steady_clock::now();
  if (int rc = ensemble_enqueue(e, mode, probs)) {
    e->scored = false;  // (the outputs of the last aggregation are gone: nothing for sfw_ensemble_blend to read)
    return rc;
  }
  e->us[1] = us_since(t0);
  t0 = std::chrono::steady_clock::now();
  if (const hipError_t he = wait_stream(e->b->h[0]); he != hipSuccess)
    return efail(e, SFW_ERR_HIP, std::string("ensemble_aggregate: ") + hipGetErrorString(he));
  for (sfw_handle h : e->b->h) stream_is_idle(h);
  if (int rc = ensemble_finish(e, costs_out, rejected_out, best_out)) return rc;
  e->us[2] = us_since(t0);
  return SFW_OK;
}

int sfw_ensemble_set_risk(sfw_ensemble e, const sfw_risk *r) {
  if (!e) return SFW_ERR_INVALID_ARG;
  if (!r) {
    e->risk = sfw_risk{1.0, 0.0, 0};
    e->risk_on = false;
    return SFW_OK;
  }
  if (!std::isfinite(r->tail_mass) || !(r->tail_mass > 0.0 && r->tail_mass <= 1.0))
    return efail(e, SFW_ERR_INVALID_ARG, "ensemble_set_risk: tail_mass must be finite, > 0 and <= 1");
  if (!std::isfinite(r->contact_mass) || !(r->contact_mass >= 0.0 && r->contact_mass < 1.0))
    return efail(e, SFW_ERR_INVALID_ARG, "ensemble_set_risk: contact_mass must be finite, >= 0 and < 1");
  if (r->reserved != 0) return efail(e, SFW_ERR_INVALID_ARG, "ensemble_set_risk: reserved must be 0");
  e->risk = *r;
  e->risk_on = true;
  return SFW_OK;
}

int sfw_ensemble_get_risk(sfw_ensemble e, sfw_risk *out, int32_t *active_out) {
  if (!e || !out) return SFW_ERR_INVALID_ARG;
  *out = e->risk;
  if (active_out) *active_out = e->risk_on ? 1 : 0;
  return SFW_OK;
}

int sfw_ensemble_set_list_fusion(sfw_ensemble e, int32_t enabled) {
  if (!e) return SFW_ERR_INVALID_ARG;
  return sfw_batch_set_list_fusion(e->b, enabled);
}

int sfw_ensemble_get_list_fusion(sfw_ensemble e, int32_t *enabled_out) {
  if (!e) return SFW_ERR_INVALID_ARG;
  return sfw_batch_get_list_fusion(e->b, enabled_out);
}

int sfw_ensemble_batch_desc(sfw_ensemble e, sfw_batch_desc *out, int64_t *table_uploads_out) {
  if (!e || !out) return SFW_ERR_INVALID_ARG;
  if (!e->b->launched) return efail(e, SFW_ERR_STATE, "ensemble_batch_desc: nothing launched");
  *out = e->b->desc;
  if (table_uploads_out) *table_uploads_out = e->chain_uploads;
  return SFW_OK;
}

int sfw_ensemble_last_us(sfw_ensemble e, int32_t which, double *us_out) {
  if (!e || !us_out) return SFW_ERR_INVALID_ARG;
  if (which < 0 || which > 2) return efail(e, SFW_ERR_INVALID_ARG, "ensemble_last_us: which must be 0..2");
  *us_out = e->us[which];
  return SFW_OK;
}

}  // extern "C"
