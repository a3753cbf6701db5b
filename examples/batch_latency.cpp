// batch_latency.cpp — B robots' control cycles (the reference's 5 x 9 grid, N pedestrians, O laser points, S steps) scored
// three ways through the C ABI; medians of the wall-clock of one cycle for ALL B robots:
//   (a) B blocking sfw_score_grid calls on one handle (the world of robot i is the same scene, its own robot state / goal);
//   (b) B handles: stage + launch all, then fetch all;
//   (c) one sfw_batch: sfw_batch_score_grid, split into stage / enqueue / wait + fetch (sfw_batch_last_us).
//
//   build: make -C social_force_window_planner_amd/csrc batchlatency
//   run:   build/batch_latency [cycles]
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

struct world {
  std::vector<uint8_t> cells;
  std::vector<double> fp, laser;
  std::vector<sfw_agent> ag;
};
static const unsigned kN = 200;
static const double kRes = 0.05, kOrigin = -5.0;

static world make_world(int n_people, int n_laser) {
  world w;
  w.cells.assign(static_cast<size_t>(kN) * kN, 0);
  for (unsigned i = 0; i < kN; ++i) w.cells[i] = w.cells[(kN - 1) * kN + i] = w.cells[i * kN] = w.cells[i * kN + kN - 1] = 255;
  for (int k = 0; k < 16; ++k) {
    w.fp.push_back(0.35 * std::cos(k * M_PI / 8));
    w.fp.push_back(0.35 * std::sin(k * M_PI / 8));
  }
  for (int i = 0; i < n_laser; ++i) {  // a wall 1.5 m to the left and a pillar ahead (as cycle_latency.cpp)
    const double u = (i + 0.5) / n_laser;
    if (i % 3) { w.laser.push_back(-2.0 + 5.0 * u); w.laser.push_back(1.5); }
    else { w.laser.push_back(2.5 + 0.2 * std::cos(9.0 * u)); w.laser.push_back(-1.0 + 0.2 * std::sin(9.0 * u)); }
  }
  w.ag.resize(1 + n_people);
  w.ag[0] = sfw_agent{};
  w.ag[0].vx = 0.3; w.ag[0].desired_velocity = 0.7; w.ag[0].radius = 0.35; w.ag[0].id = 0; w.ag[0].group_id = -1;
  for (int i = 1; i <= n_people; ++i) {
    const double a = i * 2.399963, r = 1.5 + 3.0 * i / (n_people + 1.0);
    sfw_agent q{};
    q.x = r * std::cos(a); q.y = r * std::sin(a);
    q.vx = 0.8 * std::cos(a + 2.0); q.vy = 0.8 * std::sin(a + 2.0);
    q.goal_x = q.x + 2.0 * q.vx; q.goal_y = q.y + 2.0 * q.vy;
    q.goal_radius = 0.35; q.desired_velocity = 1.0; q.radius = 0.35; q.has_goal = 1; q.id = i; q.group_id = -1;
    w.ag[i] = q;
  }
  return w;
}
static int load(sfw_handle h, const world &w) {
  int rc = sfw_set_costmap(h, w.cells.data(), kN, kN, kOrigin, kOrigin, kRes);
  rc |= sfw_set_footprint(h, w.fp.data(), 16);
  rc |= sfw_set_agents(h, w.ag.data(), static_cast<int>(w.ag.size()), w.laser.empty() ? nullptr : w.laser.data(),
                       static_cast<int>(w.laser.size() / 2));
  return rc;
}

int main(int argc, char **argv) {
  const int cycles = argc > 1 ? std::atoi(argv[1]) : 30;
  const double lin[5] = {0.0, 0.175, 0.35, 0.525, 0.7};
  const double ang[9] = {0.0, 0.125, -0.125, 0.25, -0.25, 0.375, -0.375, 0.5, -0.5};
  std::printf("per cycle of all B robots, medians of %d cycles (us): (a) B x sfw_score_grid, (b) B handles, (c) sfw_batch "
              "[stage + enqueue + wait/fetch]\n", cycles);
  for (double sim_time : {1.0, 1.5})
    for (int n_laser : {0, 60})
      for (int n_people : {0, 5, 20, 50}) {
        sfw_params p;
        sfw_params_default(&p);
        p.sim_time = sim_time;
        p.sim_granularity = sim_time == 1.0 ? 0.025 : 0.25;
        const int S = static_cast<int>(p.sim_time / p.sim_granularity + 0.5);
        const world w = make_world(n_people, n_laser);
        for (int B : {1, 4, 8, 16, 22, 32, 64}) {
          std::vector<sfw_robot_state> rs(B);
          std::vector<sfw_goal_args> ga(B);
          for (int i = 0; i < B; ++i) {
            rs[i] = sfw_robot_state{0.01 * (i % 7), -0.01 * (i % 5), 0.02 * (i % 3), 0.3 - 0.01 * (i % 4), 0.0, 0.02 * (i % 3)};
            ga[i] = sfw_goal_args{1.0, 0.0, 1.0, 2.0 + 0.1 * (i % 4), 0.5 - 0.05 * (i % 3)};
          }
          std::vector<sfw_best> best(B);
          std::vector<double> costs(45);
          // (a)
          sfw_handle one = nullptr;
          if (sfw_create(&p, 0, &one) != SFW_OK || load(one, w) != SFW_OK) {
            std::fprintf(stderr, "sfw_create / world failed (no HIP device?)\n");
            return 1;
          }
          std::vector<double> ta, tb, tc, t0s, t1s, t2s;
          for (int c = 0; c < cycles + 5; ++c) {
            const auto t0 = clk::now();
            for (int i = 0; i < B; ++i)
              if (sfw_score_grid(one, &rs[i], lin, 5, ang, 9, &ga[i], costs.data(), &best[i]) != SFW_OK) return 1;
            if (c >= 5) ta.push_back(us_since(t0));
          }
          sfw_destroy(one);
          // (b)
          std::vector<sfw_handle> hs(B, nullptr);
          for (int i = 0; i < B; ++i)
            if (sfw_create(&p, 0, &hs[i]) != SFW_OK || load(hs[i], w) != SFW_OK) return 1;
          for (int c = 0; c < cycles + 5; ++c) {
            const auto t0 = clk::now();
            for (int i = 0; i < B; ++i)
              if (sfw_grid_stage(hs[i], &rs[i], lin, 5, ang, 9, &ga[i], 0) != SFW_OK || sfw_grid_launch(hs[i]) != SFW_OK) return 1;
            for (int i = 0; i < B; ++i)
              if (sfw_grid_fetch(hs[i], costs.data(), &best[i], nullptr) != SFW_OK) return 1;
            if (c >= 5) tb.push_back(us_since(t0));
          }
          for (sfw_handle h : hs) sfw_destroy(h);
          // (c)
          sfw_batch bt = nullptr;
          if (sfw_batch_create(&p, 0, B, &bt) != SFW_OK) return 1;
          for (int i = 0; i < B; ++i)
            if (load(sfw_batch_member(bt, i), w) != SFW_OK) return 1;
          for (int c = 0; c < cycles + 5; ++c) {
            const auto t0 = clk::now();
            if (sfw_batch_score_grid(bt, rs.data(), lin, 5, ang, 9, ga.data(), best.data()) != SFW_OK) {
              std::fprintf(stderr, "batch: %s\n", sfw_batch_last_error(bt));
              return 1;
            }
            const double t = us_since(t0);
            double u0 = 0, u1 = 0, u2 = 0;
            sfw_batch_last_us(bt, 0, &u0);
            sfw_batch_last_us(bt, 1, &u1);
            sfw_batch_last_us(bt, 2, &u2);
            if (c >= 5) { tc.push_back(t); t0s.push_back(u0); t1s.push_back(u1); t2s.push_back(u2); }
          }
          sfw_batch_desc d{};
          sfw_batch_describe(bt, &d);
          sfw_batch_destroy(bt);
          std::printf("B=%2d N=%2d O=%2d S=%2d: (a) %8.1f  (b) %8.1f  (c) %8.1f [%6.1f + %6.1f + %6.1f]  per robot (c) %6.1f"
                      "  launches %d blocks %lld  best[0] %lld\n",
                      B, n_people, n_laser, S, median(ta), median(tb), median(tc), median(t0s), median(t1s), median(t2s),
                      median(tc) / B, d.batch_launches, static_cast<long long>(d.batch_blocks), static_cast<long long>(best[0].index));
          std::fflush(stdout);
        }
      }
  return 0;
}
