// ensemble_risk.cpp — a risk sweep over ONE scored grid: the grid is scored once under M crowd hypotheses, then
// sfw_ensemble_set_risk + sfw_ensemble_aggregate try five tail masses and two contact masses on it, no rollout in between.
// Per setting: the selected command, the valid samples and the median wall-clock of the re-aggregation, next to a plain
// SFW_ENSEMBLE_MEAN re-aggregation (no risk set: the unchanged kernels) on the same ensemble in the same run.
//   cases: the 5 x 9 grid with M = 4; 256 x 256 with M = 8; 256 x 256 with M = 64 (the longest walk at tail_mass = 1)
//
//   build: make -C social_force_window_planner_amd/csrc ensemblerisk
//   run:   build/ensemble_risk [repetitions]
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

// the world of examples/ensemble_latency.cpp: a walled square map, a 16-gon footprint, people on a spiral
struct world {
  unsigned n = 0;
  std::vector<uint8_t> cells;
  std::vector<double> fp;
  std::vector<sfw_agent> ag;
};

static world make_world(int n_people, unsigned n_cells) {
  world w;
  w.n = n_cells;
  w.cells.assign(static_cast<size_t>(n_cells) * n_cells, 0);
  for (unsigned i = 0; i < n_cells; ++i)
    w.cells[i] = w.cells[(n_cells - 1) * n_cells + i] = w.cells[i * n_cells] = w.cells[i * n_cells + n_cells - 1] = 255;
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

// hypothesis m: naive goal time 1 + m % 4 s, heading turned by 0.3 * (m / 4) rad, alternating sign; every fourth one has a
// person more, walking towards the robot from ahead (contact in some crowds only: what contact_mass is about)
static std::vector<sfw_agent> hypothesis(const std::vector<sfw_agent> &ag, int m) {
  std::vector<sfw_agent> h = ag;
  const double t = 1.0 + m % 4, d = 0.3 * (m / 4) * ((m / 4) % 2 ? 1.0 : -1.0), c = std::cos(d), s = std::sin(d);
  for (size_t i = 1; i < h.size(); ++i) {
    if (d != 0.0) {
      const double vx = h[i].vx, vy = h[i].vy;
      h[i].vx = c * vx - s * vy;
      h[i].vy = s * vx + c * vy;
    }
    h[i].goal_x = h[i].x + t * h[i].vx;
    h[i].goal_y = h[i].y + t * h[i].vy;
  }
  if (m % 4 == 3) {
    sfw_agent q{};
    q.x = 1.8; q.y = 0.1 * (m / 4); q.vx = -1.3; q.vy = 0.0;
    q.goal_x = q.x + 2.0 * q.vx; q.goal_y = q.y;
    q.goal_radius = 0.35; q.desired_velocity = 1.0; q.radius = 0.35; q.has_goal = 1; q.id = 90 + m; q.group_id = -1;
    h.push_back(q);
  }
  return h;
}

int main(int argc, char **argv) {
  const int reps = argc > 1 ? std::atoi(argv[1]) : 300;
  if (reps < 1) return 1;
  std::printf("risk sweep over one scored grid: sfw_ensemble_set_risk + sfw_ensemble_aggregate, medians of %d calls (us), next to the "
              "plain SFW_ENSEMBLE_MEAN re-aggregation of the same ensemble\n", reps);
  struct grid_case { int nv, nw, n_people; unsigned cells; int M; };
  const grid_case cases[] = {{5, 9, 5, 200, 4}, {256, 256, 50, 500, 8}, {256, 256, 50, 500, 64}};
  const double tails[5] = {1.0, 0.5, 0.25, 0.125, 0.05}, contacts[2] = {0.0, 0.3};
  for (const grid_case &gc : cases) {
    std::vector<double> lin(gc.nv), ang(gc.nw);
    if (gc.nv == 5 && gc.nw == 9) {
      for (int i = 0; i < 5; ++i) lin[i] = 0.175 * i;
      const double a9[9] = {0.0, 0.125, -0.125, 0.25, -0.25, 0.375, -0.375, 0.5, -0.5};
      std::copy(a9, a9 + 9, ang.begin());
    } else {  // synthetic.generalised_sampler
      for (int i = 0; i < gc.nv; ++i) lin[i] = i * (0.7 / (gc.nv - 1));
      const double s = 0.5 / (gc.nw / 2);
      for (int i = 1; i <= gc.nw / 2; ++i) { ang[2 * i - 2] = (i - 0.5) * s; ang[2 * i - 1] = (i - 0.5) * (-s); }
    }
    const world w = make_world(gc.n_people, gc.cells);
    const double origin = -(gc.cells * 0.05) / 2.0;
    sfw_params p;
    sfw_params_default(&p);
    const sfw_robot_state rs{0.0, 0.0, 0.0, 0.3, 0.0, 0.0};
    const sfw_goal_args ga{1.0, 0.0, 1.0, 2.0, 0.5};
    sfw_ensemble e = nullptr;
    if (sfw_ensemble_create(&p, 0, gc.M, &e) != SFW_OK) {
      std::fprintf(stderr, "sfw_ensemble_create failed (no HIP device?)\n");
      return 1;
    }
    if (sfw_ensemble_set_costmap(e, w.cells.data(), w.n, w.n, origin, origin, 0.05) != SFW_OK ||
        sfw_ensemble_set_footprint(e, w.fp.data(), 16) != SFW_OK)
      return 1;
    for (int m = 0; m < gc.M; ++m) {
      const std::vector<sfw_agent> h = hypothesis(w.ag, m);
      if (sfw_ensemble_set_hypothesis(e, m, h.data(), static_cast<int>(h.size()), nullptr, 0) != SFW_OK) return 1;
    }
    sfw_best plain{}, best{};
    if (sfw_ensemble_score_grid(e, &rs, lin.data(), gc.nv, ang.data(), gc.nw, &ga, SFW_ENSEMBLE_MEAN, nullptr, nullptr, nullptr, &plain) !=
        SFW_OK) {
      std::fprintf(stderr, "ensemble: %s\n", sfw_ensemble_last_error(e));
      return 1;
    }
    // one setting: the median of `reps` re-aggregations behind three that are not counted (r null: the plain aggregation)
    auto timed = [&](const sfw_risk *r, sfw_best *out) {
      if (sfw_ensemble_set_risk(e, r) != SFW_OK) return -1.0;
      std::vector<double> us;
      for (int c = 0; c < reps + 3; ++c) {
        const auto t0 = clk::now();
        if (sfw_ensemble_aggregate(e, SFW_ENSEMBLE_MEAN, nullptr, nullptr, nullptr, out) != SFW_OK) return -1.0;
        if (c >= 3) us.push_back(us_since(t0));
      }
      return median(us);
    };
    const double plain_us = timed(nullptr, &plain);
    if (plain_us < 0.0) return 1;
    std::printf("grid %3dx%-3d N=%2d M=%2d: plain MEAN %8.1f us, command (%.4f, %.4f), %lld valid\n", gc.nv, gc.nw, gc.n_people, gc.M,
                plain_us, plain.vx, plain.vtheta, static_cast<long long>(plain.n_valid));
    for (const double contact : contacts)
      for (const double tail : tails) {
        const sfw_risk r{tail, contact, 0};
        const double us = timed(&r, &best);
        if (us < 0.0) {
          std::fprintf(stderr, "ensemble: %s\n", sfw_ensemble_last_error(e));
          return 1;
        }
        std::printf("    tail_mass %-5g contact_mass %-3g: %8.1f us (x %.2f of plain), command (%.4f, %.4f), cost %.6g, %lld valid\n", tail,
                    contact, us, us / plain_us, best.vx, best.vtheta, best.cost, static_cast<long long>(best.n_valid));
        std::fflush(stdout);
      }
    // the plain aggregation once more, behind the sweep (same session, same ensemble)
    const double again_us = timed(nullptr, &best);
    std::printf("    plain MEAN again %8.1f us; same command as before the sweep: %s\n", again_us,
                best.index == plain.index && best.cost == plain.cost ? "yes" : "NO");
    sfw_ensemble_destroy(e);
    if (best.index != plain.index || best.cost != plain.cost) return 2;
  }
  return 0;
}
