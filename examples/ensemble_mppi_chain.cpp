// ensemble_mppi_chain.cpp — I MPPI iterations with the control-cost term under M crowd hypotheses, through the C ABI, two ways:
//   (a) the loop a caller had before sfw_ensemble_mppi_run: per iteration sfw_ensemble_score_perturbed with
//       SFW_PERTURB_KEEP_NORMALS (every member draws the knots), sfw_sequences_normals from member 0 (3 K n doubles over the
//       bus), the bias gamma * c_t formed on the host in the order the header defines, sfw_ensemble_blend with that bias (n
//       doubles back up), the new nominal copied;
//   (b) sfw_ensemble_mppi_run: the same iterations chained on the device behind one wait.
// Scene of mppi_chain.cpp; hypothesis m lets the people walk at (1 + 0.15 m) times their speed.  K = 8, M = 1, 4, 8,
// n = 1024 and 65 536, I = 1, 2, 4, 8; the median wall-clock of both over `repetitions` runs, same process, same ensemble,
// interleaved, and the bytes the caller moves over the bus.  The two final plans must be equal bit for bit (the host forms the
// bias without contraction: build with -ffp-contract=off), else the exit code is 2.
//
//   build: make -C social_force_window_planner_amd/csrc ensemblemppichain
//   run:   build/ensemble_mppi_chain [repetitions]        (default 30)
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

#define CHECK(e, call)                                                     \
  do {                                                                     \
    if ((call) != SFW_OK) {                                                \
      std::fprintf(stderr, "%s: %s\n", #call, sfw_ensemble_last_error(e)); \
      return 1;                                                            \
    }                                                                      \
  } while (0)

int main(int argc, char **argv) {
  const int reps = argc > 1 ? std::max(1, std::atoi(argv[1])) : 30;
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
  const double origin = -(n_cells * 0.05) / 2.0;
  std::printf("MPPI iterations under M crowd hypotheses chained on the device: %d people, %d steps, K = %d knots, MEAN, lambda 0.5, "
              "gamma 0.5, medians of %d repetitions (us)\n", people, S, K, reps);
  std::printf("%2s %8s %3s | %12s %12s %8s | %10s %10s | %14s %14s | %s\n", "M", "n", "I", "(a) loop", "(b) chain", "a / b", "(a) / iter",
              "(b) / iter", "(a) bus bytes", "(b) bus bytes", "plans");
  bool same = true;
  const double sigma[3] = {0.15, 0.05, 0.2};
  for (int M : {1, 4, 8}) {
    sfw_ensemble e = nullptr;
    if (sfw_ensemble_create(&p, 0, M, &e) != SFW_OK) {
      std::fprintf(stderr, "sfw_ensemble_create failed (no HIP device?)\n");
      return 1;
    }
    CHECK(e, sfw_ensemble_set_costmap(e, cells.data(), n_cells, n_cells, origin, origin, 0.05));
    CHECK(e, sfw_ensemble_set_footprint(e, fp.data(), 16));
    for (int m = 0; m < M; ++m) {
      const double speed = 1.0 + 0.15 * m;
      std::vector<sfw_agent> ag(1 + people);
      ag[0] = sfw_agent{};
      ag[0].vx = 0.3; ag[0].desired_velocity = 0.7; ag[0].radius = 0.35; ag[0].id = 0; ag[0].group_id = -1;
      for (int i = 1; i <= people; ++i) {
        const double a = i * 2.399963, r = 1.5 + 3.0 * i / (people + 1.0);
        sfw_agent q{};
        q.x = r * std::cos(a); q.y = r * std::sin(a);
        q.vx = speed * 0.8 * std::cos(a + 2.0); q.vy = speed * 0.8 * std::sin(a + 2.0);
        q.goal_x = q.x + 2.0 * q.vx; q.goal_y = q.y + 2.0 * q.vy;
        q.goal_radius = 0.35; q.desired_velocity = speed; q.radius = 0.35; q.has_goal = 1; q.id = i; q.group_id = -1;
        ag[i] = q;
      }
      CHECK(e, sfw_ensemble_set_hypothesis(e, m, ag.data(), static_cast<int>(ag.size()), nullptr, 0));
    }
    sfw_handle h0 = sfw_ensemble_member(e, 0);
    for (int32_t n : {1024, 65536}) {
      std::vector<double> z(static_cast<size_t>(3) * K * n), bias(n);
      for (int I : {1, 2, 4, 8}) {
        sfw_perturb pt{};
        for (int c = 0; c < 3; ++c) pt.sigma[c] = sigma[c];
        pt.lo[0] = 0.0; pt.lo[1] = -0.3; pt.lo[2] = -0.5;
        pt.hi[0] = 0.7; pt.hi[1] = 0.3; pt.hi[2] = 0.5;
        sfw_mppi mp{};
        mp.iterations = I;
        mp.lambda = 0.5;
        mp.gamma = 0.5;
        std::vector<double> nom0(3 * K, 0.0), nom(3 * K), u(3 * K), plans(static_cast<size_t>(I) * 3 * K), plan_a(3 * K);
        for (int k = 0; k < K; ++k) nom0[3 * k] = 0.3;
        std::vector<sfw_blend_stat> stats(I);
        std::vector<double> ta, tb;
        for (int rep = 0; rep < reps + 2; ++rep) {
          const uint64_t seed = 0xD1B54A32D192ED03ULL * static_cast<uint64_t>(rep + 1) + static_cast<uint64_t>(n);
          // (a) the loop of existing calls
          auto t0 = clk::now();
          nom = nom0;
          for (int i = 0; i < I; ++i) {
            sfw_best best{};
            sfw_blend_stat st{};
            pt.seed = seed + static_cast<uint64_t>(i);
            pt.nominal = nom.data();
            pt.flags = SFW_PERTURB_KEEP_NOMINAL | SFW_PERTURB_KEEP_NORMALS;
            CHECK(e, sfw_ensemble_score_perturbed(e, &rs, &pt, n, K, knot_step, &ga, SFW_ENSEMBLE_MEAN, nullptr, nullptr, nullptr, &best));
            if (sfw_sequences_normals(h0, 0, n, z.data()) != SFW_OK) {
              std::fprintf(stderr, "sfw_sequences_normals: %s\n", sfw_last_error(h0));
              return 1;
            }
            for (int32_t t = 0; t < n; ++t) {
              double acc = 0.0;
              for (int k = 0; k < K; ++k)
                for (int c = 0; c < 3; ++c) {
                  if (!(sigma[c] > 0.0)) continue;
                  const double q = nom[3 * k + c] / sigma[c];
                  acc = acc + q * z[(static_cast<size_t>(k) * 3 + c) * n + t];
                }
              bias[t] = mp.gamma * acc;
            }
            CHECK(e, sfw_ensemble_blend(e, &mp.lambda, 1, bias.data(), &st, u.data(), nullptr));
            if (st.n_valid > 0) nom = u;
          }
          const double a_us = us_since(t0);
          plan_a = nom;
          // (b) the chain
          pt.seed = seed;
          pt.nominal = nom0.data();
          pt.flags = SFW_PERTURB_KEEP_NOMINAL;
          sfw_best best{};
          t0 = clk::now();
          CHECK(e, sfw_ensemble_mppi_run(e, &rs, &pt, n, K, knot_step, &ga, SFW_ENSEMBLE_MEAN, nullptr, &mp, stats.data(), plans.data(),
                                         nullptr, nullptr, &best));
          const double b_us = us_since(t0);
          if (rep >= 2) {
            ta.push_back(a_us);
            tb.push_back(b_us);
          }
          same = same && std::memcmp(plan_a.data(), plans.data() + static_cast<size_t>(I - 1) * 3 * K, sizeof(double) * 3 * K) == 0;
          if (stats[I - 1].n_valid == 0) {
            std::fprintf(stderr, "no valid rollout at M = %d, n = %d\n", M, n);
            return 2;
          }
        }
        // what the caller moves per call: (a) per iteration the nominal, the normals down, the bias up, stat + plan down;
        // (b) the nominal once, stat + plan per iteration down
        const size_t out = sizeof(sfw_blend_stat) + sizeof(double) * 3 * K;
        const size_t bytes_a = static_cast<size_t>(I) * (sizeof(double) * 3 * K + sizeof(double) * 3 * K * n + sizeof(double) * n + out);
        const size_t bytes_b = sizeof(double) * 3 * K + static_cast<size_t>(I) * out;
        std::printf("%2d %8d %3d | %12.1f %12.1f %8.2f | %10.1f %10.1f | %14zu %14zu | %s\n", M, n, I, median(ta), median(tb),
                    median(ta) / median(tb), median(ta) / I, median(tb) / I, bytes_a, bytes_b, same ? "bitwise equal" : "DIFFER");
        std::fflush(stdout);
      }
    }
    sfw_ensemble_destroy(e);
  }
  return same ? 0 : 2;
}
