// mppi_step.cpp — a warm-started MPPI loop on a synthetic scene, through the C ABI.  Every iteration perturbs the nominal
// K-knot plan on the host (n rollouts), scores them as command sequences and takes the softmin update on the device:
//   sfw_sequences_stage + sfw_grid_launch + sfw_grid_fetch(h, NULL, &best, NULL) + sfw_grid_blend
// The blended plan — at the temperature whose effective sample size is nearest to n / 8 when L > 1 — becomes the next nominal
// plan and is scored again as an n = 1 sequence.  For n = 1024 and n = 65 536, K = 8, L = 1 and 8, the median wall-clock of
//   the blend call | the path it replaces: sfw_grid_fetch of the cost vector + the same reduction on the host
// — same process, same handle, same launch, interleaved; the two results are compared (they differ by the two exps and the
// order of summation only).
//
//   build: make -C social_force_window_planner_amd/csrc mppi
//   run:   build/mppi_step [iterations]        (default 30)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../include/sfw_hip.h"

using clk = std::chrono::steady_clock;
static double us_since(clk::time_point t0) { return std::chrono::duration<double, std::micro>(clk::now() - t0).count(); }
static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

// xorshift64* and Box-Muller: the perturbations need no more
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

// the host path: the definition of include/sfw_hip.h over the fetched cost vector, in sample order
static void host_blend(const std::vector<double> &costs, const std::vector<double> &vx, const std::vector<double> &vy,
                       const std::vector<double> &vth, int32_t n, int K, const double *lambda, int L, std::vector<double> &eta,
                       std::vector<double> &sw2, std::vector<double> &u, std::vector<double> &w) {
  double j_min = std::numeric_limits<double>::infinity();
  for (int32_t t = 0; t < n; ++t)
    if (costs[t] >= 0.0 && costs[t] < j_min) j_min = costs[t];
  for (int l = 0; l < L; ++l) {
    double e = 0.0, s2 = 0.0;
    for (int32_t t = 0; t < n; ++t) {
      const double wt = costs[t] >= 0.0 ? std::exp(-((costs[t] - j_min) / lambda[l])) : 0.0;
      w[t] = wt;
      e += wt;
      s2 += wt * wt;
    }
    eta[l] = e;
    sw2[l] = s2;
    for (int k = 0; k < K; ++k) {
      double a = 0.0, b = 0.0, c = 0.0;
      const double *px = vx.data() + static_cast<size_t>(k) * n, *py = vy.data() + static_cast<size_t>(k) * n,
                   *pt = vth.data() + static_cast<size_t>(k) * n;
      for (int32_t t = 0; t < n; ++t) {
        a += w[t] * px[t];
        b += w[t] * py[t];
        c += w[t] * pt[t];
      }
      double *o = u.data() + (static_cast<size_t>(l) * K + k) * 3;
      o[0] = e > 0.0 ? a / e : 0.0;
      o[1] = e > 0.0 ? b / e : 0.0;
      o[2] = e > 0.0 ? c / e : 0.0;
    }
  }
}

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
  std::printf("MPPI step: %d people, %d steps, K = %d knots, medians of %d iterations (us)\n", people, S, K, iters);
  std::printf("%8s %3s | %12s %18s %8s | %12s %12s | %s\n", "n", "L", "blend", "fetch + host", "ratio", "score+fetch", "max |du|",
              "cost of the blended plan: first -> last");
  double worst = 0.0;
  for (int32_t n : {1024, 65536}) {
    for (int L : {1, 8}) {
      double lambda[SFW_BLEND_MAX_L];
      for (int l = 0; l < L; ++l) lambda[l] = L == 1 ? 0.5 : 0.02 * std::pow(2.0, l);  // 0.02 .. 2.56
      std::vector<double> nom(3 * K, 0.0);  // [k][vx, vy, vtheta]
      for (int k = 0; k < K; ++k) nom[3 * k] = 0.3;
      const size_t kn = static_cast<size_t>(K) * n;
      std::vector<double> vx(kn), vy(kn), vth(kn), costs(n), w(n), u_dev(static_cast<size_t>(L) * K * 3), u_host(u_dev.size()),
          eta(L), sw2(L);
      std::vector<sfw_blend_stat> st(L);
      std::vector<double> t_blend, t_host, t_score;
      rng64 rng{0x9E3779B97F4A7C15ULL + static_cast<uint64_t>(n) * 31 + L};
      double first_cost = 0.0, last_cost = 0.0, du = 0.0;
      for (int it = 0; it < iters + 2; ++it) {
        for (int k = 0; k < K; ++k)
          for (int32_t t = 0; t < n; ++t) {
            const size_t i = static_cast<size_t>(k) * n + t;
            const double keep = t == 0 ? 0.0 : 1.0;  // sample 0 is the nominal plan itself
            vx[i] = std::min(0.7, std::max(0.0, nom[3 * k] + keep * 0.15 * rng.normal()));
            vy[i] = std::min(0.3, std::max(-0.3, nom[3 * k + 1] + keep * 0.05 * rng.normal()));
            vth[i] = std::min(0.5, std::max(-0.5, nom[3 * k + 2] + keep * 0.2 * rng.normal()));
          }
        sfw_best best{};
        auto t0 = clk::now();
        CHECK(h, sfw_sequences_stage(h, &rs, vx.data(), vy.data(), vth.data(), n, K, knot_step, &ga, 0));
        CHECK(h, sfw_grid_launch(h));
        CHECK(h, sfw_grid_fetch(h, nullptr, &best, nullptr));
        const double a_score = us_since(t0);
        t0 = clk::now();
        CHECK(h, sfw_grid_blend(h, lambda, L, nullptr, st.data(), u_dev.data(), nullptr));
        const double a_blend = us_since(t0);
        t0 = clk::now();
        CHECK(h, sfw_grid_fetch(h, costs.data(), nullptr, nullptr));
        host_blend(costs, vx, vy, vth, n, K, lambda, L, eta, sw2, u_host, w);
        const double a_host = us_since(t0);
        if (it >= 2) {
          t_blend.push_back(a_blend);
          t_host.push_back(a_host);
          t_score.push_back(a_score);
        }
        for (size_t i = 0; i < u_dev.size(); ++i) du = std::max(du, std::fabs(u_dev[i] - u_host[i]));
        if (st[0].n_valid == 0) {
          std::fprintf(stderr, "no valid rollout at n = %d\n", n);
          return 2;
        }
        // the temperature whose effective sample size is nearest to n / 8
        int pick = 0;
        double miss = std::numeric_limits<double>::infinity();
        for (int l = 0; l < L; ++l) {
          const double ess = st[l].eta * st[l].eta / st[l].sum_w2, m = std::fabs(ess - n / 8.0);
          if (m < miss) {
            miss = m;
            pick = l;
          }
        }
        for (int i = 0; i < 3 * K; ++i) nom[i] = u_dev[static_cast<size_t>(pick) * K * 3 + i];
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
      worst = std::max(worst, du);
      std::printf("%8d %3d | %12.1f %18.1f %8.2f | %12.1f %12.2e | %.6f -> %.6f\n", n, L, median(t_blend), median(t_host),
                  median(t_host) / median(t_blend), median(t_score), du, first_cost, last_cost);
      std::fflush(stdout);
    }
  }
  sfw_destroy(h);
  const bool ok = worst <= 1e-9;
  std::printf("%s\n", ok ? "device and host blends agree (max |du| <= 1e-9)" : "BLEND MISMATCH");
  return ok ? 0 : 2;
}
