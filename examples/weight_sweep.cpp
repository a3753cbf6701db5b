// weight_sweep.cpp — what a weight sweep costs through the C ABI: the scoring step with term capture off and on, then
// sfw_grid_rescore of K weight vectors over the captured terms against K fresh sfw_score_grid calls (sfw_set_params with
// each vector, then the blocking call).  Medians of the wall-clock of the blocking calls, on two grids:
//   target  256 x 256 samples, 50 people, 40 steps (the flagship grid of bench.py)
//   cycle   the reference's 5 x 9 samples (src/sfw_planner.cpp:64-85), 5 people, 40 steps
// Every re-scored selection is checked field for field against its fresh score ("match" in the last column).
//
//   build: make -C social_force_window_planner_amd/csrc weightsweep
//   run:   build/weight_sweep [reps]
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
#define CHECK(call)                                                                   \
  do {                                                                                \
    const int rc_ = (call);                                                           \
    if (rc_ != SFW_OK) {                                                              \
      std::fprintf(stderr, "%s failed: %d (%s)\n", #call, rc_, sfw_last_error(h));    \
      std::exit(1);                                                                   \
    }                                                                                 \
  } while (0)

struct grid {
  const char *name;
  std::vector<double> lin, ang;
  int people;
};

static const unsigned kN = 400;
static const double kRes = 0.05, kOrigin = -10.0;

static void load_world(sfw_handle h, int n_people) {
  std::vector<uint8_t> cells(static_cast<size_t>(kN) * kN, 0);
  for (unsigned i = 0; i < kN; ++i) cells[i] = cells[(kN - 1) * kN + i] = cells[i * kN] = cells[i * kN + kN - 1] = 255;
  for (unsigned y = 40; y < 60; ++y)  // an obstacle block ahead-left: some samples end on illegal cells
    for (unsigned x = 250; x < 275; ++x) cells[y * kN + x] = 254;
  for (unsigned y = 150; y < 250; ++y)  // a cost gradient
    for (unsigned x = 220; x < 260; ++x) cells[y * kN + x] = static_cast<uint8_t>((x - 220) * 5);
  std::vector<double> fp;
  for (int k = 0; k < 16; ++k) {
    fp.push_back(0.35 * std::cos(k * M_PI / 8));
    fp.push_back(0.35 * std::sin(k * M_PI / 8));
  }
  std::vector<sfw_agent> ag(1 + n_people);
  ag[0] = sfw_agent{};
  ag[0].vx = 0.3; ag[0].desired_velocity = 0.7; ag[0].radius = 0.35; ag[0].id = 0; ag[0].group_id = -1;
  for (int i = 1; i <= n_people; ++i) {
    const double a = i * 2.399963, r = 1.5 + 6.0 * i / (n_people + 1.0);
    sfw_agent q{};
    q.x = r * std::cos(a); q.y = r * std::sin(a);
    q.vx = 0.8 * std::cos(a + 2.0); q.vy = 0.8 * std::sin(a + 2.0);
    q.goal_x = q.x + 2.0 * q.vx; q.goal_y = q.y + 2.0 * q.vy;
    q.goal_radius = 0.35; q.desired_velocity = 1.0; q.radius = 0.35; q.has_goal = 1; q.id = i; q.group_id = -1;
    ag[i] = q;
  }
  CHECK(sfw_set_costmap(h, cells.data(), kN, kN, kOrigin, kOrigin, kRes));
  CHECK(sfw_set_footprint(h, fp.data(), 16));
  CHECK(sfw_set_agents(h, ag.data(), static_cast<int32_t>(ag.size()), nullptr, 0));
}

static bool same_best(const sfw_best &a, const sfw_best &b) {
  return a.index == b.index && std::memcmp(&a.cost, &b.cost, sizeof(double)) == 0 && a.vx == b.vx && a.vy == b.vy &&
         a.vtheta == b.vtheta && a.n_valid == b.n_valid;
}

static void run(const grid &g, int reps) {
  sfw_params p;
  sfw_params_default(&p);
  sfw_handle h = nullptr;
  if (sfw_create(&p, 0, &h) != SFW_OK) {
    std::fprintf(stderr, "sfw_create failed (no GPU?)\n");
    std::exit(1);
  }
  load_world(h, g.people);
  const sfw_robot_state rs{0.0, 0.0, 0.1, 0.3, 0.0, 0.05};
  const sfw_goal_args ga{2.5, 0.0, 3.2, 3.0, 1.0};
  const int nv = static_cast<int>(g.lin.size()), nw = static_cast<int>(g.ang.size());
  const size_t T = static_cast<size_t>(nv) * nw;
  std::vector<double> costs(T);
  sfw_best best;
  auto score = [&]() {
    const auto t0 = clk::now();
    CHECK(sfw_score_grid(h, &rs, g.lin.data(), nv, g.ang.data(), nw, &ga, costs.data(), &best));
    return us_since(t0);
  };
  for (int i = 0; i < 3; ++i) score();
  std::vector<double> off, on;
  for (int i = 0; i < reps; ++i) off.push_back(score());
  CHECK(sfw_set_terms_capture(h, 1));
  for (int i = 0; i < 3; ++i) score();
  for (int i = 0; i < reps; ++i) on.push_back(score());
  // the same two once more, interleaved, against drift of the clock between the two blocks
  std::vector<double> off2, on2;
  for (int i = 0; i < reps; ++i) {
    CHECK(sfw_set_terms_capture(h, 0));
    off2.push_back(score());
    CHECK(sfw_set_terms_capture(h, 1));
    on2.push_back(score());
  }
  const double m_off = median(off), m_on = median(on), m_off2 = median(off2), m_on2 = median(on2);
  std::printf("%-7s %d x %d samples, %d people, %d steps\n", g.name, nv, nw, g.people, static_cast<int>(p.sim_time / p.sim_granularity + 0.5));
  std::printf("  sfw_score_grid  capture off  %10.1f us   capture on %10.1f us   (%+.2f %%)\n", m_off, m_on, 100.0 * (m_on / m_off - 1.0));
  std::printf("  (interleaved)   capture off  %10.1f us   capture on %10.1f us   (%+.2f %%)\n", m_off2, m_on2, 100.0 * (m_on2 / m_off2 - 1.0));
  // the capturing launch every re-score reads (the default weights)
  score();
  std::vector<sfw_weights> W;
  srand(7);
  auto u = [] { return 3.0 * rand() / RAND_MAX; };
  for (int k = 0; k < 256; ++k) W.push_back(sfw_weights{u(), u(), u(), u(), u()});
  std::printf("  %4s %16s %16s %20s %8s\n", "K", "rescore us", "per vector us", "K fresh scores us", "match");
  for (int K : {1, 16, 256}) {
    std::vector<sfw_best> rb(K);
    std::vector<double> ts;
    for (int i = 0; i < reps; ++i) {
      const auto t0 = clk::now();
      CHECK(sfw_grid_rescore(h, W.data(), K, rb.data(), nullptr));
      ts.push_back(us_since(t0));
    }
    const double m_rs = median(ts);
    // K fresh scores on a second handle (the first keeps the captured launch)
    sfw_handle h2 = nullptr;
    CHECK(sfw_create(&p, 0, &h2));
    load_world(h2, g.people);
    std::vector<double> c2(T);
    sfw_best b2;
    bool match = true;
    const auto t0 = clk::now();
    for (int k = 0; k < K; ++k) {
      sfw_params pk = p;
      pk.vel_weight = W[k].vel; pk.distance_weight = W[k].distance; pk.angle_weight = W[k].angle;
      pk.costmap_weight = W[k].costmap; pk.social_weight = W[k].social;
      CHECK(sfw_set_params(h2, &pk));
      CHECK(sfw_score_grid(h2, &rs, g.lin.data(), nv, g.ang.data(), nw, &ga, c2.data(), &b2));
      match = match && same_best(b2, rb[k]);
    }
    const double fresh = us_since(t0);
    sfw_destroy(h2);
    std::printf("  %4d %16.1f %16.2f %20.1f %8s\n", K, m_rs, m_rs / K, fresh, match ? "yes" : "NO");
  }
  sfw_destroy(h);
}

int main(int argc, char **argv) {
  const int reps = argc > 1 ? std::max(3, std::atoi(argv[1])) : 21;
  grid target{"target", {}, {}, 50};
  for (int i = 0; i < 256; ++i) target.lin.push_back(0.7 * i / 255.0);
  for (int i = 0; i < 256; ++i) target.ang.push_back(-0.5 + 1.0 * i / 255.0);
  grid cycle{"cycle", {0.0, 0.175, 0.35, 0.525, 0.7}, {0.0, 0.125, -0.125, 0.25, -0.25, 0.375, -0.375, 0.5, -0.5}, 5};
  run(target, reps);
  run(cycle, reps);
  return 0;
}
