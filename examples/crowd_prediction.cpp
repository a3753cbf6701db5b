// crowd_prediction.cpp — the pedestrian prediction behind the winning command: the reference's 5 x 9 grid
// (src/sfw_planner.cpp:64-85) on a 5-person scene, then sfw_grid_crowd of the winner: per person the social work it
// contributes (Wp summed over the steps), the minimum clearance to the robot and the step at which it occurs — and what the
// dump costs next to the robot's own Trajectory points (sfw_grid_points) for the same sample, medians of 300 calls.
//
//   build: make -C social_force_window_planner_amd/csrc crowd
//   run:   build/crowd_prediction [calls]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/sfw_hip.h"

using clk = std::chrono::steady_clock;
static double us_since(clk::time_point t0) {
  return std::chrono::duration<double, std::micro>(clk::now() - t0).count();
}
static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char **argv) {
  const int calls = argc > 1 ? std::atoi(argv[1]) : 300;
  const unsigned N = 200;
  const double res = 0.05, origin = -5.0;
  std::vector<uint8_t> cells(static_cast<size_t>(N) * N, 0);
  for (unsigned i = 0; i < N; ++i) cells[i] = cells[(N - 1) * N + i] = cells[i * N] = cells[i * N + N - 1] = 255;
  std::vector<double> fp;
  for (int k = 0; k < 16; ++k) {
    fp.push_back(0.35 * std::cos(k * M_PI / 8));
    fp.push_back(0.35 * std::sin(k * M_PI / 8));
  }
  const double lin[5] = {0.0, 0.175, 0.35, 0.525, 0.7};
  const double ang[9] = {0.0, 0.125, -0.125, 0.25, -0.25, 0.375, -0.375, 0.5, -0.5};
  const sfw_robot_state rs{0.0, 0.0, 0.0, 0.3, 0.0, 0.0};
  const sfw_goal_args ga{1.0, 0.0, 1.0, 2.0, 0.5};
  const int n_people = 5, A = 1 + n_people;

  sfw_params p;
  sfw_params_default(&p);
  sfw_handle h = nullptr;
  if (sfw_create(&p, 0, &h) != SFW_OK) {
    std::fprintf(stderr, "sfw_create failed (no HIP device?)\n");
    return 1;
  }
  std::vector<sfw_agent> ag(A);
  ag[0] = sfw_agent{};
  ag[0].vx = 0.3; ag[0].desired_velocity = 0.7; ag[0].radius = 0.35; ag[0].id = 0; ag[0].group_id = -1;
  for (int i = 1; i <= n_people; ++i) {
    const double a = i * 2.399963, r = 1.5 + 3.0 * i / (n_people + 1.0);
    sfw_agent q{};
    q.x = r * std::cos(a); q.y = r * std::sin(a);
    q.vx = 0.8 * std::cos(a + 2.0); q.vy = 0.8 * std::sin(a + 2.0);
    q.goal_x = q.x + 2.0 * q.vx; q.goal_y = q.y + 2.0 * q.vy;
    q.goal_radius = 0.35; q.desired_velocity = 1.0; q.radius = 0.35; q.has_goal = 1; q.id = i; q.group_id = -1;
    ag[i] = q;
  }
  const int S = static_cast<int>(p.sim_time / p.sim_granularity + 0.5);
  std::vector<double> costs(45);
  sfw_best best;
  int rc = sfw_set_costmap(h, cells.data(), N, N, origin, origin, res);
  rc |= sfw_set_footprint(h, fp.data(), 16);
  rc |= sfw_set_agents(h, ag.data(), A, nullptr, 0);
  rc |= sfw_score_grid(h, &rs, lin, 5, ang, 9, &ga, costs.data(), &best);
  if (rc != SFW_OK || best.index < 0) {
    std::fprintf(stderr, "error: %s\n", rc != SFW_OK ? sfw_last_error(h) : "no selectable sample");
    return 1;
  }

  std::vector<double> state(static_cast<size_t>(S) * A * 4), work(static_cast<size_t>(S) * A), pts(static_cast<size_t>(S) * 3);
  std::vector<int32_t> hg(static_cast<size_t>(S) * A);
  double cost = 0.0;
  int32_t n = 0, np = 0;
  if (sfw_grid_crowd(h, best.index, &cost, state.data(), work.data(), hg.data(), A, S, &n) != SFW_OK) {
    std::fprintf(stderr, "error: %s\n", sfw_last_error(h));
    return 1;
  }
  std::printf("winner: sample %lld  cmd_vel (%.3f, %.3f)  cost %.6f (sfw_grid_crowd: %.6f)  %d steps of %d\n",
              static_cast<long long>(best.index), best.vx, best.vtheta, best.cost, cost, n, S);
  double wr = 0.0, total = 0.0;
  for (int i = 0; i < n; ++i) wr += work[static_cast<size_t>(i) * A];
  total = wr;
  std::printf("  robot    Wr %.6f\n", wr);
  for (int a = 1; a < A; ++a) {
    double wp = 0.0, dmin = INFINITY;
    int at = -1, popped = -1;
    for (int i = 0; i < n; ++i) {
      const size_t o = static_cast<size_t>(i) * A;
      wp += work[o + a];
      const double d = std::hypot(state[(o + a) * 4] - state[o * 4], state[(o + a) * 4 + 1] - state[o * 4 + 1]);
      if (d < dmin) { dmin = d; at = i; }
      if (popped < 0 && !hg[o + a]) popped = i;
    }
    total += wp;
    std::printf("  person %d Wp %.6f  min clearance %.3f m at step %d", a, wp, dmin, at);
    if (popped >= 0) std::printf("  (goal reached at step %d)", popped);
    std::printf("\n");
  }
  std::printf("  social work of the sample: %.6f\n", total);

  // the dump's latency next to the robot's own points, same handle, same sample
  std::vector<double> t_crowd, t_points;
  for (int c = 0; c < calls + 10; ++c) {
    auto t0 = clk::now();
    rc = sfw_grid_crowd(h, best.index, &cost, state.data(), work.data(), hg.data(), A, S, &n);
    const double a = us_since(t0);
    t0 = clk::now();
    rc |= sfw_grid_points(h, best.index, pts.data(), S, &np);
    const double b = us_since(t0);
    if (rc != SFW_OK) {
      std::fprintf(stderr, "error: %s\n", sfw_last_error(h));
      return 1;
    }
    if (c >= 10) { t_crowd.push_back(a); t_points.push_back(b); }
  }
  std::printf("A=%d S=%d: sfw_grid_crowd %6.1f us  sfw_grid_points %6.1f us  (medians of %d; %d bytes of rows)\n", A, S,
              median(t_crowd), median(t_points), calls, 44 * n * A);
  sfw_destroy(h);
  return 0;
}
