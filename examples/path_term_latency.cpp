// path_term_latency.cpp — what sfw_set_path costs: the wall-clock of one blocking sfw_score_grid without a path and with a
// path of 16 / 64 / 1024 points (weight 2.0), medians with the middle half's width as the run-to-run spread, the settings
// interleaved call by call, at
//   (a) the reference's 5 x 9 grid with 0 / 5 / 20 people — where a path also means leaving the one-launch kernel, so the step
//       is timed a third way: no path, one-launch kernel off (SFW_CYCLE_FUSED=0): (path - that) is the term's three kernels,
//       (that - off) the kernel left;
//   (b) the target configuration: 256 x 256 samples, 50 people, 500 x 500 cells: no path against a 64-point path.
// Every cost is compared with off + weight * p (one product, one sum), bit for bit, p read back by sfw_grid_path_term.
//
//   build: make -C social_force_window_planner_amd/csrc pathterm
//   run:   build/path_term_latency [cycles]
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
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

// a global plan of n points: a gentle left bend of 4 m that starts half a metre behind the robot
static std::vector<double> make_path(int n) {
  std::vector<double> xy;
  for (int i = 0; i < n; ++i) {
    const double s = n > 1 ? static_cast<double>(i) / (n - 1) : 0.0;
    xy.push_back(-0.5 + 4.0 * s);
    xy.push_back(0.6 * s * s);
  }
  return xy;
}

#define CHECK(h, call)                                                  \
  do {                                                                  \
    if ((call) != SFW_OK) {                                             \
      std::fprintf(stderr, "%s: %s\n", #call, sfw_last_error(h));       \
      return 1;                                                         \
    }                                                                   \
  } while (0)

static int run(const char *name, int nv, int nw, int n_people, unsigned n_cells, int cycles, bool small, const std::vector<int> &sizes,
               int *mismatches) {
  sfw_params p;
  sfw_params_default(&p);
  const sfw_robot_state rs{0.0, 0.0, 0.0, 0.3, 0.0, 0.0};
  const sfw_goal_args ga{1.0, 0.0, 1.0, 2.0, 0.5};
  const double weight = 2.0, origin = -(n_cells * 0.05) / 2.0;
  std::vector<uint8_t> cells(static_cast<size_t>(n_cells) * n_cells, 0);
  std::vector<double> fp;
  for (int k = 0; k < 16; ++k) {
    fp.push_back(0.35 * std::cos(k * M_PI / 8));
    fp.push_back(0.35 * std::sin(k * M_PI / 8));
  }
  std::vector<sfw_agent> ag(static_cast<size_t>(n_people > 0 ? 1 + n_people : 0));
  if (n_people > 0) {
    ag[0] = sfw_agent{};
    ag[0].vx = 0.3; ag[0].desired_velocity = 0.7; ag[0].radius = 0.35; ag[0].id = 0; ag[0].group_id = -1;
  }
  for (int i = 1; i <= n_people; ++i) {
    const double a = i * 2.399963, r = 1.5 + 3.0 * i / (n_people + 1.0);
    sfw_agent q{};
    q.x = r * std::cos(a); q.y = r * std::sin(a);
    q.vx = 0.8 * std::cos(a + 2.0); q.vy = 0.8 * std::sin(a + 2.0);
    q.goal_x = q.x + 2.0 * q.vx; q.goal_y = q.y + 2.0 * q.vy;
    q.goal_radius = 0.35; q.desired_velocity = 1.0; q.radius = 0.35; q.has_goal = 1; q.id = i; q.group_id = -1;
    ag[static_cast<size_t>(i)] = q;
  }
  sfw_handle h = nullptr;
  if (sfw_create(&p, 0, &h) != SFW_OK) {
    std::fprintf(stderr, "sfw_create failed (no HIP device?)\n");
    return 1;
  }
  CHECK(h, sfw_set_costmap(h, cells.data(), n_cells, n_cells, origin, origin, 0.05));
  CHECK(h, sfw_set_footprint(h, fp.data(), 16));
  CHECK(h, sfw_set_agents(h, ag.empty() ? nullptr : ag.data(), static_cast<int>(ag.size()), nullptr, 0));
  std::vector<double> lin(nv), ang(nw);
  for (int i = 0; i < nv; ++i) lin[i] = i * (0.7 / (nv - 1));
  ang[0] = 0.0;
  for (int j = 1; j < nw; ++j) ang[j] = ((j + 1) / 2) * (0.5 / (nw / 2)) * ((j & 1) ? 1.0 : -1.0);
  const int64_t T = static_cast<int64_t>(nv) * nw;
  std::vector<double> off(T), unf(T), on(T), term(T);
  std::vector<std::vector<double>> paths;
  for (int n : sizes) paths.push_back(make_path(n));
  std::vector<double> t_off, t_unf;
  std::vector<std::vector<double>> t_on(sizes.size());
  sfw_best b{};
  int64_t differ = 0;
  for (int c = 0; c < cycles + 3; ++c) {
    CHECK(h, sfw_set_path(h, nullptr));
    auto t0 = clk::now();
    CHECK(h, sfw_score_grid(h, &rs, lin.data(), nv, ang.data(), nw, &ga, off.data(), &b));
    if (c >= 3) t_off.push_back(us_since(t0));
    if (small) {  // no path, the kernels one by one
      setenv("SFW_CYCLE_FUSED", "0", 1);
      t0 = clk::now();
      CHECK(h, sfw_score_grid(h, &rs, lin.data(), nv, ang.data(), nw, &ga, unf.data(), &b));
      if (c >= 3) t_unf.push_back(us_since(t0));
      unsetenv("SFW_CYCLE_FUSED");
    }
    for (size_t k = 0; k < sizes.size(); ++k) {
      const sfw_path path{paths[k].data(), sizes[k], 0, weight};
      CHECK(h, sfw_set_path(h, &path));
      t0 = clk::now();
      CHECK(h, sfw_score_grid(h, &rs, lin.data(), nv, ang.data(), nw, &ga, on.data(), &b));
      if (c >= 3) t_on[k].push_back(us_since(t0));
      if (c == 0) {  // once per size: the cost is off + weight * p, bit for bit
        CHECK(h, sfw_grid_path_term(h, 0, T, term.data()));
        for (int64_t t = 0; t < T; ++t) {
          volatile double prod = weight * term[t];  // (rounded on its own: no contraction with the sum)
          const double want = (term[t] >= 0.0 && off[t] != SFW_COST_INVALID) ? off[t] + prod : off[t];
          if (!same_bits(on[t], want) || (small && !same_bits(unf[t], off[t]))) ++differ;
        }
      }
    }
  }
  *mismatches += differ ? 1 : 0;
  std::printf("%-7s %3d x %3d, %2d people | no path %9.1f (spread %6.1f)", name, nv, nw, n_people, median(t_off), spread(t_off));
  if (small) std::printf(" | without the one-launch kernel %8.1f (leaving it %+.1f us)", median(t_unf), median(t_unf) - median(t_off));
  for (size_t k = 0; k < sizes.size(); ++k) {
    std::printf(" | %4d points %9.1f (spread %6.1f, %+.1f us", sizes[k], median(t_on[k]), spread(t_on[k]), median(t_on[k]) - median(t_off));
    if (small) std::printf(", the term %+.1f us", median(t_on[k]) - median(t_unf));
    std::printf(")");
  }
  std::printf(" | %lld costs differ\n", static_cast<long long>(differ));
  std::fflush(stdout);
  sfw_destroy(h);
  return 0;
}

int main(int argc, char **argv) {
  const int cycles = argc > 1 ? std::atoi(argv[1]) : 30;
  int mismatches = 0;
  std::printf("path term (weight 2.0), medians of blocking sfw_score_grid calls (us)\n");
  for (int people : {0, 5, 20})
    if (run("ref5x9", 5, 9, people, 200, cycles, true, {16, 64, 1024}, &mismatches)) return 1;
  // the long path once more with one thread per pose (SFW_PATH_SLICES=0, read by sfw_create): what slicing the segments over
  // the grid buys
  setenv("SFW_PATH_SLICES", "0", 1);
  if (run("1thread", 5, 9, 5, 200, cycles, true, {1024}, &mismatches)) return 1;
  unsetenv("SFW_PATH_SLICES");
  if (run("target", 256, 256, 50, 500, std::max(5, cycles / 3), false, {64}, &mismatches)) return 1;
  std::printf("%s\n", mismatches ? "COST MISMATCH" : "every cost equals the path-off cost + weight * p, bit for bit");
  return mismatches ? 2 : 0;
}
