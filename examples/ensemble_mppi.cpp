// ensemble_mppi.cpp — a risk-aware MPPI loop through the C ABI: the rollouts are drawn on the device, scored under M = 4
// naive-goal hypotheses of where the crowd is heading, aggregated (MEAN) and blended over a ladder of temperatures, all on
// the device.  Every iteration is
//   shift the nominal plan + sfw_ensemble_score_perturbed + sfw_ensemble_blend
// and sends the first knot of the blended plan.  For n = 1024 and n = 16 384 rollouts, K = 8, 5 people, the median wall-clock
// of an iteration against the path it replaces, same process, interleaved:
//   (a) M standalone handles: sfw_score_perturbed each (the same seed: the same knots), the M term vectors fetched with
//       sfw_grid_terms, the knots with sfw_sequences_knots, the ensemble definition and the softmin reduction on the host;
//   (b) the ensemble: two calls, nothing proportional to n crosses the bus.
// It also counts how often MEAN and MAX (sfw_ensemble_aggregate) choose a different first knot.
//
//   build: make -C social_force_window_planner_amd/csrc ensemblemppi
//   run:   build/ensemble_mppi [iterations]        (default 30)
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

#define CHECK(err, call)                                \
  do {                                                  \
    if ((call) != SFW_OK) {                             \
      std::fprintf(stderr, "%s: %s\n", #call, (err));   \
      return 1;                                         \
    }                                                   \
  } while (0)

int main(int argc, char **argv) {
  const int iters = std::max(1, argc > 1 ? std::atoi(argv[1]) : 30);
  sfw_params p;
  sfw_params_default(&p);
  const int S = static_cast<int>(p.sim_time / p.sim_granularity + 0.5);
  const sfw_robot_state rs{0.0, 0.0, 0.0, 0.3, 0.0, 0.0};
  const sfw_goal_args ga{1.0, 0.7, 1.0, 2.0, 0.5};
  constexpr int K = 8, people = 5, M = 4, L = 4, PLAN = 1;  // PLAN: the temperature whose mean becomes the next plan
  const double lambda[L] = {0.1, 0.5, 2.0, 10.0};
  const double goal_time[M] = {1.0, 2.0, 3.0, 4.0};
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
  // hypothesis m: every person heads for position + goal_time[m] * velocity
  std::vector<std::vector<sfw_agent>> hyp(M, std::vector<sfw_agent>(1 + people));
  for (int m = 0; m < M; ++m) {
    hyp[m][0] = sfw_agent{};
    hyp[m][0].vx = 0.3; hyp[m][0].desired_velocity = 0.7; hyp[m][0].radius = 0.35; hyp[m][0].id = 0; hyp[m][0].group_id = -1;
    for (int i = 1; i <= people; ++i) {
      const double a = i * 2.399963, r = 1.5 + 3.0 * i / (people + 1.0);
      sfw_agent q{};
      q.x = r * std::cos(a); q.y = r * std::sin(a);
      q.vx = 0.8 * std::cos(a + 2.0); q.vy = 0.8 * std::sin(a + 2.0);
      q.goal_x = q.x + goal_time[m] * q.vx; q.goal_y = q.y + goal_time[m] * q.vy;
      q.goal_radius = 0.35; q.desired_velocity = 1.0; q.radius = 0.35; q.has_goal = 1; q.id = i; q.group_id = -1;
      hyp[m][i] = q;
    }
  }
  const double origin = -(n_cells * 0.05) / 2.0;
  sfw_ensemble e = nullptr;
  if (sfw_ensemble_create(&p, 0, M, &e) != SFW_OK) {
    std::fprintf(stderr, "sfw_ensemble_create failed (no HIP device?)\n");
    return 1;
  }
  CHECK(sfw_ensemble_last_error(e), sfw_ensemble_set_costmap(e, cells.data(), n_cells, n_cells, origin, origin, 0.05));
  CHECK(sfw_ensemble_last_error(e), sfw_ensemble_set_footprint(e, fp.data(), 16));
  sfw_handle hs[M];
  for (int m = 0; m < M; ++m) {
    CHECK(sfw_ensemble_last_error(e), sfw_ensemble_set_hypothesis(e, m, hyp[m].data(), 1 + people, nullptr, 0));
    if (sfw_create(&p, 0, &hs[m]) != SFW_OK) return 1;
    CHECK(sfw_last_error(hs[m]), sfw_set_costmap(hs[m], cells.data(), n_cells, n_cells, origin, origin, 0.05));
    CHECK(sfw_last_error(hs[m]), sfw_set_footprint(hs[m], fp.data(), 16));
    CHECK(sfw_last_error(hs[m]), sfw_set_agents(hs[m], hyp[m].data(), 1 + people, nullptr, 0));
    CHECK(sfw_last_error(hs[m]), sfw_set_terms_capture(hs[m], 1));
  }
  std::printf("risk-aware MPPI: M = %d hypotheses, %d people, %d steps, K = %d knots, L = %d temperatures, medians of %d "
              "iterations\n", M, people, S, K, L, iters);
  std::printf("%8s | %16s %16s %8s | %18s %18s | %14s | %s\n", "n", "(a) handles+host", "(b) ensemble", "a / b",
              "(a) bytes over bus", "(b) bytes over bus", "MEAN != MAX", "largest |u_a - u_b|, first knot sent last");
  for (int32_t n : {1024, 16384}) {
    std::vector<double> nom(3 * K, 0.0);  // [k][vx, vy, vtheta]
    for (int k = 0; k < K; ++k) nom[3 * k] = 0.3;
    const size_t kn = static_cast<size_t>(K) * n;
    std::vector<double> terms(static_cast<size_t>(M) * n * SFW_N_TERMS), vx(kn), vy(kn), vth(kn), cost(n), w(n);
    std::vector<double> u(static_cast<size_t>(L) * K * 3), ua(static_cast<size_t>(L) * K * 3);
    std::vector<double> ta, tb;
    sfw_perturb pt{};
    pt.sigma[0] = 0.15; pt.sigma[1] = 0.05; pt.sigma[2] = 0.2;
    pt.lo[0] = 0.0; pt.lo[1] = -0.3; pt.lo[2] = -0.5;
    pt.hi[0] = 0.7; pt.hi[1] = 0.3; pt.hi[2] = 0.5;
    pt.flags = SFW_PERTURB_KEEP_NOMINAL;  // sample 0 is the nominal plan itself
    int differ = 0;
    double u_gap = 0.0;
    sfw_best sent{};
    for (int it = 0; it < iters + 2; ++it) {
      // shift: the plan moves one knot on, the last knot is kept
      for (int k = 0; k + 1 < K; ++k)
        for (int c = 0; c < 3; ++c) nom[3 * k + c] = nom[3 * (k + 1) + c];
      pt.nominal = nom.data();
      pt.seed = 0xD1B54A32D192ED03ULL * static_cast<uint64_t>(it + 1) + static_cast<uint64_t>(n);  // a new seed every cycle
      // (a) M handles, the terms and the knots to the host, the definition and the softmin there
      auto t0 = clk::now();
      for (int m = 0; m < M; ++m) {
        CHECK(sfw_last_error(hs[m]), sfw_score_perturbed(hs[m], &rs, &pt, n, K, knot_step, &ga, nullptr, nullptr));
        CHECK(sfw_last_error(hs[m]), sfw_grid_terms(hs[m], 0, n, terms.data() + static_cast<size_t>(m) * n * SFW_N_TERMS));
      }
      CHECK(sfw_last_error(hs[0]), sfw_sequences_knots(hs[0], 0, n, vx.data(), vy.data(), vth.data()));
      double j_min = INFINITY;
      for (int32_t t = 0; t < n; ++t) {
        const double *t0m = terms.data() + static_cast<size_t>(t) * SFW_N_TERMS;
        bool rejected = false;
        double acc = 0.0;
        for (int m = 0; m < M; ++m) {
          const double *tm = terms.data() + (static_cast<size_t>(m) * n + t) * SFW_N_TERMS;
          rejected = rejected || tm[SFW_TERM_DISTANCE] == SFW_COST_INVALID;
          acc = acc + (1.0 / M) * tm[SFW_TERM_SOCIAL];
        }
        double c = p.vel_weight * t0m[SFW_TERM_VEL] + p.distance_weight * t0m[SFW_TERM_DISTANCE] + p.angle_weight * t0m[SFW_TERM_ANGLE];
        c = c + p.costmap_weight * t0m[SFW_TERM_COSTMAP];
        c = std::fma(p.social_weight, acc, c);  // (the scoring kernels add the social term in one rounding)
        cost[t] = rejected ? SFW_COST_INVALID : c;
        if (!rejected) j_min = std::min(j_min, c);
      }
      for (int l = 0; l < L; ++l) {
        double eta = 0.0;
        for (int32_t t = 0; t < n; ++t) {
          w[t] = cost[t] >= 0.0 ? std::exp(-((cost[t] - j_min) / lambda[l])) : 0.0;
          eta += w[t];
        }
        for (int k = 0; k < K; ++k) {
          double sx = 0.0, sy = 0.0, sth = 0.0;
          const size_t row = static_cast<size_t>(k) * n;
          for (int32_t t = 0; t < n; ++t) {
            sx += w[t] * vx[row + t];
            sy += w[t] * vy[row + t];
            sth += w[t] * vth[row + t];
          }
          double *const o = ua.data() + (static_cast<size_t>(l) * K + k) * 3;
          o[0] = eta > 0.0 ? sx / eta : 0.0;
          o[1] = eta > 0.0 ? sy / eta : 0.0;
          o[2] = eta > 0.0 ? sth / eta : 0.0;
        }
      }
      const double t_a = us_since(t0);
      // (b) the ensemble
      sfw_best best{};
      sfw_blend_stat st[L];
      t0 = clk::now();
      CHECK(sfw_ensemble_last_error(e), sfw_ensemble_score_perturbed(e, &rs, &pt, n, K, knot_step, &ga, SFW_ENSEMBLE_MEAN, nullptr,
                                                                     nullptr, nullptr, &best));
      CHECK(sfw_ensemble_last_error(e), sfw_ensemble_blend(e, lambda, L, nullptr, st, u.data(), nullptr));
      const double t_b = us_since(t0);
      if (st[PLAN].n_valid == 0) {
        std::fprintf(stderr, "no valid rollout at n = %d\n", n);
        return 2;
      }
      if (it >= 2) {
        ta.push_back(t_a);
        tb.push_back(t_b);
      }
      for (size_t i = 0; i < u.size(); ++i) u_gap = std::max(u_gap, std::fabs(u[i] - ua[i]));
      // the worst-case choice over the same rollouts: no new rollout, one kernel
      sfw_best worst{};
      CHECK(sfw_ensemble_last_error(e), sfw_ensemble_aggregate(e, SFW_ENSEMBLE_MAX, nullptr, nullptr, nullptr, &worst));
      if (worst.index != best.index) ++differ;
      for (int i = 0; i < 3 * K; ++i) nom[i] = u[static_cast<size_t>(PLAN) * K * 3 + i];
      sent.vx = nom[0]; sent.vy = nom[1]; sent.vtheta = nom[2];
    }
    // per iteration: (a) M term vectors and the knots down, M perturbation records up; (b) the records and the blend's outputs
    const double bytes_a = static_cast<double>(M) * n * SFW_N_TERMS * 8 + 3.0 * K * n * 8 + M * (sizeof(sfw_perturb) + 3.0 * K * 8);
    const double bytes_b = M * (sizeof(sfw_perturb) + 3.0 * K * 8) + sizeof(sfw_best) + L * sizeof(sfw_blend_stat) + 3.0 * K * L * 8;
    std::printf("%8d | %13.1f us %13.1f us %8.2f | %18.0f %18.0f | %6d of %4d | %.3e, (%.4f, %.4f, %.4f)\n", n, median(ta),
                median(tb), median(ta) / median(tb), bytes_a, bytes_b, differ, iters + 2, u_gap, sent.vx, sent.vy, sent.vtheta);
    std::fflush(stdout);
  }
  for (int m = 0; m < M; ++m) sfw_destroy(hs[m]);
  sfw_ensemble_destroy(e);
  return 0;
}
