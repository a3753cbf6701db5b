// stop_check_latency.cpp — what sfw_set_stop_check costs: the wall-clock of one blocking sfw_score_grid with the check off and
// with it on (the host mirror's default limits, 1.0 / 1.0 / 1.0: a tail of about 28 steps of 0.025 s from 0.7 m/s), medians,
// the two settings interleaved call by call, at
//   (a) the reference's 5 x 9 grid with 5 people — where "on" also means leaving the one-launch kernel, so the step is timed a
//       third way: check off, one-launch kernel off (SFW_CYCLE_FUSED=0): (on - that) is the tail, (that - off) the kernel left;
//   (b) cfg2: 128 x 128 samples, 20 people, a 200 x 200 costmap;
//   (c) the target configuration: 256 x 256 samples, 50 people, 500 x 500 cells — with the shader clock the launches ran at.
// The samples the check leaves alone are compared with the check-off costs, bit for bit.
//
//   build: make -C social_force_window_planner_amd/csrc stopcheck
//   run:   build/stop_check_latency [cycles]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/sfw_hip.h"

using clk = std::chrono::steady_clock;
static double us_since(clk::time_point t0) { return std::chrono::duration<double, std::micro>(clk::now() - t0).count(); }
static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}
static double spread(std::vector<double> v) {  // the middle half's width: run-to-run spread without the outliers
  std::sort(v.begin(), v.end());
  return v[(3 * v.size()) / 4] - v[v.size() / 4];
}

struct world {
  unsigned n = 0;
  std::vector<uint8_t> cells;
  std::vector<double> fp;
  std::vector<sfw_agent> ag;
};

// a free map with an unknown border and a lethal ring of radius 1.0 m around the robot: beyond every rollout (0.55 m and the
// footprint's 0.35 m at most), inside the braking path of the faster samples (another 0.25 m from 0.7 m/s)
static world make_world(int n_people, unsigned n_cells) {
  world w;
  w.n = n_cells;
  w.cells.assign(static_cast<size_t>(n_cells) * n_cells, 0);
  for (unsigned i = 0; i < n_cells; ++i)
    w.cells[i] = w.cells[(n_cells - 1) * n_cells + i] = w.cells[i * n_cells] = w.cells[i * n_cells + n_cells - 1] = 255;
  const double origin = -(n_cells * 0.05) / 2.0;
  for (unsigned y = 0; y < n_cells; ++y)
    for (unsigned x = 0; x < n_cells; ++x) {
      const double d = std::hypot(origin + (x + 0.5) * 0.05, origin + (y + 0.5) * 0.05);
      if (d > 1.0 && d < 1.1) w.cells[static_cast<size_t>(y) * n_cells + x] = 254;
    }
  for (int k = 0; k < 16; ++k) {
    w.fp.push_back(0.35 * std::cos(k * M_PI / 8));
    w.fp.push_back(0.35 * std::sin(k * M_PI / 8));
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

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

#define CHECK(h, call)                                                  \
  do {                                                                  \
    if ((call) != SFW_OK) {                                             \
      std::fprintf(stderr, "%s: %s\n", #call, sfw_last_error(h));       \
      return 1;                                                         \
    }                                                                   \
  } while (0)

static int run(const char *name, int nv, int nw, int n_people, unsigned n_cells, int cycles, bool small, int *mismatches) {
  sfw_params p;
  sfw_params_default(&p);
  const sfw_robot_state rs{0.0, 0.0, 0.0, 0.3, 0.0, 0.0};
  const sfw_goal_args ga{1.0, 0.0, 1.0, 2.0, 0.5};
  const sfw_stop_check check{1.0, 1.0, 1.0, SFW_STOP_MAX_STEPS, 0};
  const world w = make_world(n_people, n_cells);
  const double origin = -(w.n * 0.05) / 2.0;
  sfw_handle h = nullptr;
  if (sfw_create(&p, 0, &h) != SFW_OK) {
    std::fprintf(stderr, "sfw_create failed (no HIP device?)\n");
    return 1;
  }
  CHECK(h, sfw_set_costmap(h, w.cells.data(), w.n, w.n, origin, origin, 0.05));
  CHECK(h, sfw_set_footprint(h, w.fp.data(), 16));
  CHECK(h, sfw_set_agents(h, w.ag.data(), static_cast<int>(w.ag.size()), nullptr, 0));
  std::vector<double> lin(nv), ang(nw);
  for (int i = 0; i < nv; ++i) lin[i] = i * (0.7 / (nv - 1));
  ang[0] = 0.0;
  for (int j = 1; j < nw; ++j) ang[j] = ((j + 1) / 2) * (0.5 / (nw / 2)) * ((j & 1) ? 1.0 : -1.0);
  const int64_t T = static_cast<int64_t>(nv) * nw;
  std::vector<double> off(T), on(T), unf(T);
  sfw_best b{};
  std::vector<double> t_off, t_on, t_unf, ghz_off, ghz_on;
  if (!small) CHECK(h, sfw_set_timing(h, 1));
  for (int c = 0; c < cycles + 3; ++c) {
    double g = 0.0;
    CHECK(h, sfw_set_stop_check(h, nullptr));
    auto t0 = clk::now();
    CHECK(h, sfw_score_grid(h, &rs, lin.data(), nv, ang.data(), nw, &ga, off.data(), &b));
    const double a = us_since(t0);
    if (!small) CHECK(h, sfw_last_clock_ghz(h, &g));
    if (c >= 3) { t_off.push_back(a); ghz_off.push_back(g); }
    if (small) {  // check off, the three-kernel path
      setenv("SFW_CYCLE_FUSED", "0", 1);
      t0 = clk::now();
      CHECK(h, sfw_score_grid(h, &rs, lin.data(), nv, ang.data(), nw, &ga, unf.data(), &b));
      if (c >= 3) t_unf.push_back(us_since(t0));
      unsetenv("SFW_CYCLE_FUSED");
    }
    CHECK(h, sfw_set_stop_check(h, &check));
    t0 = clk::now();
    CHECK(h, sfw_score_grid(h, &rs, lin.data(), nv, ang.data(), nw, &ga, on.data(), &b));
    const double d = us_since(t0);
    if (!small) CHECK(h, sfw_last_clock_ghz(h, &g));
    if (c >= 3) { t_on.push_back(d); ghz_on.push_back(g); }
  }
  std::vector<sfw_stop_rec> rec(T);
  sfw_plan_info info{};
  CHECK(h, sfw_grid_stop_info(h, 0, T, rec.data()));
  CHECK(h, sfw_grid_plan_info(h, &info));
  int64_t stopped = 0, valid_off = 0, differ = 0;
  int longest = 0;
  for (int64_t t = 0; t < T; ++t) {
    valid_off += off[t] >= 0;
    longest = std::max(longest, rec[t].steps);
    const bool rej = rec[t].hit >= 0 || rec[t].hit == SFW_STOP_UNFINISHED;
    stopped += rej;
    if (rej ? on[t] != SFW_COST_INVALID : !same_bits(on[t], off[t])) ++differ;
    if (small && !same_bits(unf[t], off[t])) ++differ;
  }
  *mismatches += differ ? 1 : 0;
  std::printf("%-7s %3d x %3d, %2d people | off %9.1f (spread %6.1f) | on %9.1f (spread %6.1f) | +%8.1f us, %+.1f %%", name, nv, nw, n_people,
              median(t_off), spread(t_off), median(t_on), spread(t_on), median(t_on) - median(t_off),
              100.0 * (median(t_on) - median(t_off)) / median(t_off));
  if (small)
    std::printf(" | off without the one-launch kernel %8.1f: leaving it %+.1f us, the tail %+.1f us", median(t_unf),
                median(t_unf) - median(t_off), median(t_on) - median(t_unf));
  else
    std::printf(" | %.2f / %.2f GHz", median(ghz_off), median(ghz_on));
  std::printf(" | %lld of %lld valid samples rejected by the check, longest tail %d steps, %d levels, %lld costs differ\n",
              static_cast<long long>(stopped), static_cast<long long>(valid_off), longest, info.levels, static_cast<long long>(differ));
  std::fflush(stdout);
  sfw_destroy(h);
  return 0;
}

int main(int argc, char **argv) {
  const int cycles = argc > 1 ? std::atoi(argv[1]) : 30;
  int mismatches = 0;
  std::printf("stop check (limits 1.0 / 1.0 / 1.0), medians of blocking sfw_score_grid calls (us)\n");
  if (run("ref5x9", 5, 9, 5, 200, cycles, true, &mismatches)) return 1;
  if (run("cfg2", 128, 128, 20, 200, std::max(5, cycles / 2), false, &mismatches)) return 1;
  if (run("target", 256, 256, 50, 500, std::max(5, cycles / 3), false, &mismatches)) return 1;
  std::printf("%s\n", mismatches ? "COST MISMATCH" : "every sample the check leaves alone equals the check-off cost, bit for bit");
  return mismatches ? 2 : 0;
}
