// batch_mppi_latency.cpp — a fleet of MPPI controllers, and one controller under crowd hypotheses, with the list-fusion switch
// on against off (sfw_batch_set_list_fusion / sfw_ensemble_set_list_fusion), through the C ABI.  5 people, S = 40, K = 8;
// medians of the wall-clock of one call, the same process and the same handles for both settings, the two settings alternating
// block by block:
//   (1) sfw_batch_score_perturbed at B in {1, 4, 22} x n in {64, 256, 1024};
//   (2) sfw_ensemble_mppi_run at M in {2, 4, 8} x n in {256, 1024}, I = 4.
// Off is the path without the switch: every member its own launch of sfw_cycle_seq_kernel.
//
//   build: make -C social_force_window_planner_amd/csrc batchmppi
//   run:   build/batch_mppi_latency [calls per setting, default 300]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/sfw_hip.h"

using clk = std::chrono::steady_clock;
static double us_since(clk::time_point t0) { return std::chrono::duration<double, std::micro>(clk::now() - t0).count(); }
static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

static const unsigned kN = 200;
static const double kRes = 0.05, kOrigin = -5.0;
static const int kK = 8, kPeople = 5;

struct world {
  std::vector<uint8_t> cells;
  std::vector<double> fp;
  std::vector<sfw_agent> ag;
};
// (the world of batch_latency.cpp; `turn` rotates the people's headings: a crowd hypothesis)
static world make_world(double turn) {
  world w;
  w.cells.assign(static_cast<size_t>(kN) * kN, 0);
  for (unsigned i = 0; i < kN; ++i) w.cells[i] = w.cells[(kN - 1) * kN + i] = w.cells[i * kN] = w.cells[i * kN + kN - 1] = 255;
  for (int k = 0; k < 16; ++k) {
    w.fp.push_back(0.35 * std::cos(k * M_PI / 8));
    w.fp.push_back(0.35 * std::sin(k * M_PI / 8));
  }
  w.ag.resize(1 + kPeople);
  w.ag[0] = sfw_agent{};
  w.ag[0].vx = 0.3; w.ag[0].desired_velocity = 0.7; w.ag[0].radius = 0.35; w.ag[0].id = 0; w.ag[0].group_id = -1;
  for (int i = 1; i <= kPeople; ++i) {
    const double a = i * 2.399963, r = 1.5 + 3.0 * i / (kPeople + 1.0);
    sfw_agent q{};
    q.x = r * std::cos(a); q.y = r * std::sin(a);
    q.vx = 0.8 * std::cos(a + 2.0 + turn); q.vy = 0.8 * std::sin(a + 2.0 + turn);
    q.goal_x = q.x + 2.0 * q.vx; q.goal_y = q.y + 2.0 * q.vy;
    q.goal_radius = 0.35; q.desired_velocity = 1.0; q.radius = 0.35; q.has_goal = 1; q.id = i; q.group_id = -1;
    w.ag[i] = q;
  }
  return w;
}

#define CHECK(call, who)                                    \
  do {                                                      \
    if ((call) != SFW_OK) {                                 \
      std::fprintf(stderr, "%s failed: %s\n", #call, who);  \
      return 1;                                             \
    }                                                       \
  } while (0)

int main(int argc, char **argv) {
  const int calls = argc > 1 ? std::atoi(argv[1]) : 300;
  const int block = 25;  // calls of one setting before the other takes its turn
  sfw_params p;
  sfw_params_default(&p);
  p.sim_time = 1.0;
  p.sim_granularity = 0.025;  // S = 40
  int32_t knot_step[kK];
  double nominal[kK * 3];
  for (int k = 0; k < kK; ++k) {
    knot_step[k] = 5 * k;
    nominal[3 * k] = 0.35 + 0.05 * std::cos(k);
    nominal[3 * k + 1] = 0.0;
    nominal[3 * k + 2] = -0.05 + 0.1 * std::sin(0.7 * k);
  }
  const world w0 = make_world(0.0);
  std::printf("medians of %d calls per setting (us), 5 people, S = 40, K = %d; desc = one_launch_members / own_path_members / "
              "batch_launches / batch_blocks / lds_bytes\n", calls, kK);
  std::printf("-- sfw_batch_score_perturbed\n");
  for (int B : {1, 4, 22})
    for (int n : {64, 256, 1024}) {
      sfw_batch bt = nullptr;
      if (sfw_batch_create(&p, 0, B, &bt) != SFW_OK) {
        std::fprintf(stderr, "sfw_batch_create failed (no HIP device?)\n");
        return 1;
      }
      std::vector<sfw_robot_state> rs(B);
      std::vector<sfw_goal_args> ga(B);
      std::vector<sfw_perturb> pt(B);
      std::vector<sfw_best> best(B);
      for (int i = 0; i < B; ++i) {
        sfw_handle h = sfw_batch_member(bt, i);
        CHECK(sfw_set_costmap(h, w0.cells.data(), kN, kN, kOrigin, kOrigin, kRes), sfw_last_error(h));
        CHECK(sfw_set_footprint(h, w0.fp.data(), 16), sfw_last_error(h));
        CHECK(sfw_set_agents(h, w0.ag.data(), static_cast<int>(w0.ag.size()), nullptr, 0), sfw_last_error(h));
        rs[i] = sfw_robot_state{0.01 * (i % 7), -0.01 * (i % 5), 0.02 * (i % 3), 0.3 - 0.01 * (i % 4), 0.0, 0.02 * (i % 3)};
        ga[i] = sfw_goal_args{1.0, 0.7, 1.0, 2.0 + 0.1 * (i % 4), 0.5 - 0.05 * (i % 3)};
        pt[i] = sfw_perturb{1000u + 17u * i, nominal, {0.2, 0.1, 0.3}, {0.0, -0.3, -0.5}, {0.7, 0.3, 0.5}, 0, 0};
      }
      std::vector<double> t[2];
      sfw_batch_desc d[2] = {};
      long long first[2] = {-2, -2};
      for (int done = -block; done < calls; done += block)  // (the first block of each setting warms up)
        for (int on = 0; on < 2; ++on) {
          CHECK(sfw_batch_set_list_fusion(bt, on), sfw_batch_last_error(bt));
          for (int c = 0; c < block; ++c) {
            const auto t0 = clk::now();
            CHECK(sfw_batch_score_perturbed(bt, rs.data(), pt.data(), n, kK, knot_step, ga.data(), best.data()), sfw_batch_last_error(bt));
            if (done >= 0) t[on].push_back(us_since(t0));
          }
          CHECK(sfw_batch_describe(bt, &d[on]), sfw_batch_last_error(bt));
          first[on] = static_cast<long long>(best[B - 1].index);
        }
      sfw_batch_destroy(bt);
      std::printf("B=%2d n=%4d: off %8.1f  on %8.1f  per robot %7.1f -> %7.1f   desc off %d/%d/%d/%lld/%d  on %d/%d/%d/%lld/%d   "
                  "winner of the last member %lld | %lld\n", B, n, median(t[0]), median(t[1]), median(t[0]) / B, median(t[1]) / B,
                  d[0].one_launch_members, d[0].own_path_members, d[0].batch_launches, static_cast<long long>(d[0].batch_blocks),
                  d[0].lds_bytes, d[1].one_launch_members, d[1].own_path_members, d[1].batch_launches,
                  static_cast<long long>(d[1].batch_blocks), d[1].lds_bytes, first[0], first[1]);
      std::fflush(stdout);
    }
  std::printf("-- sfw_ensemble_mppi_run, I = 4\n");
  for (int M : {2, 4, 8})
    for (int n : {256, 1024}) {
      sfw_ensemble e = nullptr;
      if (sfw_ensemble_create(&p, 0, M, &e) != SFW_OK) return 1;
      CHECK(sfw_ensemble_set_costmap(e, w0.cells.data(), kN, kN, kOrigin, kOrigin, kRes), sfw_ensemble_last_error(e));
      CHECK(sfw_ensemble_set_footprint(e, w0.fp.data(), 16), sfw_ensemble_last_error(e));
      for (int m = 0; m < M; ++m) {
        const world w = make_world(0.15 * m);
        CHECK(sfw_ensemble_set_hypothesis(e, m, w.ag.data(), static_cast<int>(w.ag.size()), nullptr, 0), sfw_ensemble_last_error(e));
      }
      const sfw_robot_state rs{0.0, 0.0, 0.0, 0.3, 0.0, 0.0};
      const sfw_goal_args ga{1.0, 0.7, 1.0, 2.0, 0.5};
      const sfw_perturb pt{4242u, nominal, {0.2, 0.1, 0.3}, {0.0, -0.3, -0.5}, {0.7, 0.3, 0.5}, 0, 0};
      const sfw_mppi mp{4, 0, 1.0, 0.3};
      sfw_blend_stat stat[4];
      double plans[4 * kK * 3];
      sfw_best best;
      std::vector<double> t[2];
      sfw_batch_desc d[2] = {};
      int64_t up[2] = {0, 0};
      double last_plan[2] = {0.0, 0.0};
      for (int done = -block; done < calls; done += block)
        for (int on = 0; on < 2; ++on) {
          CHECK(sfw_ensemble_set_list_fusion(e, on), sfw_ensemble_last_error(e));
          for (int c = 0; c < block; ++c) {
            const auto t0 = clk::now();
            CHECK(sfw_ensemble_mppi_run(e, &rs, &pt, n, kK, knot_step, &ga, SFW_ENSEMBLE_MEAN, nullptr, &mp, stat, plans, nullptr, nullptr,
                                        &best),
                  sfw_ensemble_last_error(e));
            if (done >= 0) t[on].push_back(us_since(t0));
          }
          CHECK(sfw_ensemble_batch_desc(e, &d[on], &up[on]), sfw_ensemble_last_error(e));
          last_plan[on] = plans[3 * kK * 3];
        }
      sfw_ensemble_destroy(e);
      std::printf("M=%d n=%4d: off %8.1f  on %8.1f  per iteration %7.1f -> %7.1f   desc off %d/%d/%d/%lld/%d  on %d/%d/%d/%lld/%d  "
                  "table uploads %lld   plan[3][0].vx %.17g | %.17g\n", M, n, median(t[0]), median(t[1]), median(t[0]) / 4, median(t[1]) / 4,
                  d[0].one_launch_members, d[0].own_path_members, d[0].batch_launches, static_cast<long long>(d[0].batch_blocks),
                  d[0].lds_bytes, d[1].one_launch_members, d[1].own_path_members, d[1].batch_launches,
                  static_cast<long long>(d[1].batch_blocks), d[1].lds_bytes, static_cast<long long>(up[1]), last_plan[0], last_plan[1]);
      std::fflush(stdout);
    }
  return 0;
}
