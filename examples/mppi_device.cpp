// mppi_device.cpp — the loop of mppi_step.cpp with the rollouts drawn on the device, through the C ABI.  Every iteration is
//   sfw_sequences_perturb_stage + sfw_grid_launch + sfw_grid_fetch(h, NULL, &best, NULL) + sfw_grid_blend
// — a nominal plan of 3 K doubles, three standard deviations, a clamp box and a seed go in, the blended plan comes out; no
// K x n array exists on the host.  For n = 1024 and n = 65 536, K = 8, 5 people, the median wall-clock of
//   (a) the host path: the draw exactly as mppi_step.cpp does it (xorshift64* + Box-Muller, one core) + sfw_sequences_stage
//   (b) the device path: sfw_sequences_perturb_stage
// each up to the return of the stage call and up to the return of sfw_grid_fetch — same process, same handle, interleaved.
// In the first iteration of every case the knots the device drew are read back (sfw_sequences_knots) and staged by
// sfw_sequences_stage: the selection must be the perturbed stage's bit for bit.
//
//   build: make -C social_force_window_planner_amd/csrc mppidev
//   run:   build/mppi_device [iterations]        (default 30)
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

// xorshift64* and Box-Muller: the host draw of mppi_step.cpp
struct rng64 {
  uint64_t s;
  double uniform() {
    s ^= s >> 12;
    s ^= s << 25;
    s ^= s >> 27;
    return static_cast<double>((s * 0x2545F4914F6CDD1DULL) >> 11) * (1.0 / 9007199254740992.0);
  }
  double normal() {
    const double u1 = std::max(uniform(), 1e-300), u2 = uniform();
    return std::sqrt(-2.0 * std::log(u1)) * std::cos(2.0 * M_PI * u2);
  }
};

#define CHECK(h, call)                                                  \
  do {                                                                  \
    if ((call) != SFW_OK) {                                             \
      std::fprintf(stderr, "%s: %s\n", #call, sfw_last_error(h));       \
      return 1;                                                         \
    }                                                                   \
  } while (0)

int main(int argc, char **argv) {
  const int iters = argc > 1 ? std::atoi(argv[1]) : 30;
  sfw_params p;
  sfw_params_default(&p);
  const int S = static_cast<int>(p.sim_time / p.sim_granularity + 0.5);
  const sfw_robot_state rs{0.0, 0.0, 0.0, 0.3, 0.0, 0.0};
  const sfw_goal_args ga{1.0, 0.7, 1.0, 2.0, 0.5};
  const int K = 8, people = 5;
  int32_t knot_step[K];
  for (int k = 0; k < K; ++k) knot_step[k] = k * S / K;
  const unsigned n_cells = 200;
  std::vector<uint8_t> cells(static_cast<size_t>(n_cells) * n_cells, 0);
  for (unsigned i = 0; i < n_cells; ++i)
    cells[i] = cells[(n_cells - 1) * n_cells + i] = cells[i * n_cells] = cells[i * n_cells + n_cells - 1] = 255;
  std::vector<double> fp;
  for (int k = 0; k < 16; ++k) {
    fp.push_back(0.35 * std::cos(k * M_PI / 8));
    fp.push_back(0.35 * std::sin(k * M_PI / 8));
  }
  std::vector<sfw_agent> ag(1 + people);
  ag[0] = sfw_agent{};
  ag[0].vx = 0.3; ag[0].desired_velocity = 0.7; ag[0].radius = 0.35; ag[0].id = 0; ag[0].group_id = -1;
  for (int i = 1; i <= people; ++i) {
    const double a = i * 2.399963, r = 1.5 + 3.0 * i / (people + 1.0);
    sfw_agent q{};
    q.x = r * std::cos(a); q.y = r * std::sin(a);
    q.vx = 0.8 * std::cos(a + 2.0); q.vy = 0.8 * std::sin(a + 2.0);
    q.goal_x = q.x + 2.0 * q.vx; q.goal_y = q.y + 2.0 * q.vy;
    q.goal_radius = 0.35; q.desired_velocity = 1.0; q.radius = 0.35; q.has_goal = 1; q.id = i; q.group_id = -1;
    ag[i] = q;
  }
  sfw_handle h = nullptr;
  const double origin = -(n_cells * 0.05) / 2.0;
  if (sfw_create(&p, 0, &h) != SFW_OK) {
    std::fprintf(stderr, "sfw_create failed (no HIP device?)\n");
    return 1;
  }
  CHECK(h, sfw_set_costmap(h, cells.data(), n_cells, n_cells, origin, origin, 0.05));
  CHECK(h, sfw_set_footprint(h, fp.data(), 16));
  CHECK(h, sfw_set_agents(h, ag.data(), static_cast<int>(ag.size()), nullptr, 0));
  std::printf("MPPI on the device: %d people, %d steps, K = %d knots, medians of %d iterations (us)\n", people, S, K, iters);
  std::printf("%8s | %14s %14s %8s | %14s %14s %8s | %s\n", "n", "(a) draw+stage", "(b) perturb", "a / b", "(a) .. fetch",
              "(b) .. fetch", "a / b", "cost of the blended plan: first -> last");
  bool same = true;
  for (int32_t n : {1024, 65536}) {
    const double lambda[1] = {0.5};
    std::vector<double> nom(3 * K, 0.0);  // [k][vx, vy, vtheta]
    for (int k = 0; k < K; ++k) nom[3 * k] = 0.3;
    const size_t kn = static_cast<size_t>(K) * n;
    std::vector<double> vx(kn), vy(kn), vth(kn), u(static_cast<size_t>(K) * 3);
    std::vector<double> a_stage, a_fetch, b_stage, b_fetch;
    rng64 rng{0x9E3779B97F4A7C15ULL + static_cast<uint64_t>(n) * 31};
    sfw_perturb pt{};
    pt.nominal = nom.data();
    pt.sigma[0] = 0.15; pt.sigma[1] = 0.05; pt.sigma[2] = 0.2;
    pt.lo[0] = 0.0; pt.lo[1] = -0.3; pt.lo[2] = -0.5;
    pt.hi[0] = 0.7; pt.hi[1] = 0.3; pt.hi[2] = 0.5;
    pt.flags = SFW_PERTURB_KEEP_NOMINAL;  // sample 0 is the nominal plan itself
    double first_cost = 0.0, last_cost = 0.0;
    for (int it = 0; it < iters + 2; ++it) {
      sfw_best best_a{}, best_b{};
      // (a) the host path
      auto t0 = clk::now();
      for (int k = 0; k < K; ++k)
        for (int32_t t = 0; t < n; ++t) {
          const size_t i = static_cast<size_t>(k) * n + t;
          const double keep = t == 0 ? 0.0 : 1.0;
          vx[i] = std::min(0.7, std::max(0.0, nom[3 * k] + keep * 0.15 * rng.normal()));
          vy[i] = std::min(0.3, std::max(-0.3, nom[3 * k + 1] + keep * 0.05 * rng.normal()));
          vth[i] = std::min(0.5, std::max(-0.5, nom[3 * k + 2] + keep * 0.2 * rng.normal()));
        }
      CHECK(h, sfw_sequences_stage(h, &rs, vx.data(), vy.data(), vth.data(), n, K, knot_step, &ga, 0));
      const double ta_stage = us_since(t0);
      CHECK(h, sfw_grid_launch(h));
      CHECK(h, sfw_grid_fetch(h, nullptr, &best_a, nullptr));
      const double ta_fetch = us_since(t0);
      // (b) the device path
      pt.seed = 0xD1B54A32D192ED03ULL * static_cast<uint64_t>(it + 1) + static_cast<uint64_t>(n);  // a new seed every cycle
      t0 = clk::now();
      CHECK(h, sfw_sequences_perturb_stage(h, &rs, &pt, n, K, knot_step, &ga, 0));
      const double tb_stage = us_since(t0);
      CHECK(h, sfw_grid_launch(h));
      CHECK(h, sfw_grid_fetch(h, nullptr, &best_b, nullptr));
      const double tb_fetch = us_since(t0);
      if (it >= 2) {
        a_stage.push_back(ta_stage);
        a_fetch.push_back(ta_fetch);
        b_stage.push_back(tb_stage);
        b_fetch.push_back(tb_fetch);
      }
      sfw_blend_stat st{};
      CHECK(h, sfw_grid_blend(h, lambda, 1, nullptr, &st, u.data(), nullptr));
      if (st.n_valid == 0) {
        std::fprintf(stderr, "no valid rollout at n = %d\n", n);
        return 2;
      }
      if (it == 0) {  // what the device drew, staged by the host: the same selection, bit for bit
        CHECK(h, sfw_sequences_knots(h, 0, n, vx.data(), vy.data(), vth.data()));
        sfw_best again{};
        CHECK(h, sfw_score_sequences(h, &rs, vx.data(), vy.data(), vth.data(), n, K, knot_step, &ga, nullptr, &again));
        same = same && std::memcmp(&again, &best_b, sizeof(again)) == 0;
      }
      for (int i = 0; i < 3 * K; ++i) nom[i] = u[i];
      // the blended plan as an n = 1 sequence
      std::vector<double> bx(K), by(K), bth(K);
      for (int k = 0; k < K; ++k) {
        bx[k] = nom[3 * k];
        by[k] = nom[3 * k + 1];
        bth[k] = nom[3 * k + 2];
      }
      double c1 = 0.0;
      CHECK(h, sfw_score_sequences(h, &rs, bx.data(), by.data(), bth.data(), 1, K, knot_step, &ga, &c1, nullptr));
      if (it == 0) first_cost = c1;
      last_cost = c1;
    }
    std::printf("%8d | %14.1f %14.1f %8.2f | %14.1f %14.1f %8.2f | %.6f -> %.6f\n", n, median(a_stage), median(b_stage),
                median(a_stage) / median(b_stage), median(a_fetch), median(b_fetch), median(a_fetch) / median(b_fetch), first_cost,
                last_cost);
    std::fflush(stdout);
  }
  sfw_destroy(h);
  std::printf("%s\n", same ? "the host-staged knots of the device draw select what the perturbed stage selected"
                           : "SELECTION MISMATCH");
  return same ? 0 : 2;
}
