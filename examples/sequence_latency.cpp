// sequence_latency.cpp — command SEQUENCES (sfw_score_sequences: K knots per sample, the command changes inside the horizon)
// against the sample list of the same size (sfw_score_samples), through the C ABI.  For n = 45, 512 and 2100 samples at 5 and
// 20 people and 40 steps: the median wall-clock of one blocking call of
//   a K = 4 sequence stage | a K = 1 sequence stage | the list of the same n
// — all three in the same process on the same handle, interleaved.  The K = 1 costs are checked against the list's and a
// K = 4 stage of constant sequences against it too, bit for bit.
//
//   build: make -C social_force_window_planner_amd/csrc sequences
//   run:   build/sequence_latency [calls]        (default 300)
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
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

#define CHECK(h, call)                                                  \
  do {                                                                  \
    if ((call) != SFW_OK) {                                             \
      std::fprintf(stderr, "%s: %s\n", #call, sfw_last_error(h));       \
      return 1;                                                         \
    }                                                                   \
  } while (0)

int main(int argc, char **argv) {
  const int calls = argc > 1 ? std::atoi(argv[1]) : 300;
  sfw_params p;
  sfw_params_default(&p);
  const int S = static_cast<int>(p.sim_time / p.sim_granularity + 0.5);
  const sfw_robot_state rs{0.0, 0.0, 0.0, 0.3, 0.0, 0.0};
  const sfw_goal_args ga{1.0, 0.7, 1.0, 2.0, 0.5};
  const int K = 4;
  const int32_t knot_step[K] = {0, S / 4, S / 2, 3 * S / 4};
  const unsigned n_cells = 200;
  std::vector<uint8_t> cells(static_cast<size_t>(n_cells) * n_cells, 0);
  for (unsigned i = 0; i < n_cells; ++i)
    cells[i] = cells[(n_cells - 1) * n_cells + i] = cells[i * n_cells] = cells[i * n_cells + n_cells - 1] = 255;
  std::vector<double> fp;
  for (int k = 0; k < 16; ++k) {
    fp.push_back(0.35 * std::cos(k * M_PI / 8));
    fp.push_back(0.35 * std::sin(k * M_PI / 8));
  }
  int mismatches = 0;
  std::printf("command sequences, %d steps, medians of %d blocking calls (us)\n", S, calls);
  std::printf("%8s %8s | %12s %12s %12s | %s\n", "people", "n", "K = 4", "K = 1", "list", "K = 4 / list");
  for (int people : {5, 20}) {
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
    for (int32_t n : {45, 512, 2100}) {
      // knot 0: a fan of commands; knots 1..3: the same fan turned further, so that every sample's command really changes
      std::vector<double> vx(static_cast<size_t>(K) * n), vth(static_cast<size_t>(K) * n), cx(static_cast<size_t>(K) * n),
          cth(static_cast<size_t>(K) * n);
      for (int k = 0; k < K; ++k)
        for (int32_t t = 0; t < n; ++t) {
          const double lin = 0.7 * ((t * 7) % 11) / 10.0, ang = -0.5 + 1.0 * ((t * 3) % 17) / 16.0;
          vx[static_cast<size_t>(k) * n + t] = std::max(0.0, lin - 0.1 * k);
          vth[static_cast<size_t>(k) * n + t] = ang * (1.0 - 0.25 * k);
          cx[static_cast<size_t>(k) * n + t] = lin;
          cth[static_cast<size_t>(k) * n + t] = ang;
        }
      std::vector<double> c4(n), c1(n), cl(n), cc(n);
      sfw_best b{};
      std::vector<double> t4, t1, tl;
      for (int c = 0; c < calls + 3; ++c) {
        auto t0 = clk::now();
        CHECK(h, sfw_score_sequences(h, &rs, vx.data(), nullptr, vth.data(), n, K, knot_step, &ga, c4.data(), &b));
        const double a4 = us_since(t0);
        t0 = clk::now();
        CHECK(h, sfw_score_sequences(h, &rs, vx.data(), nullptr, vth.data(), n, 1, knot_step, &ga, c1.data(), &b));
        const double a1 = us_since(t0);
        t0 = clk::now();
        CHECK(h, sfw_score_samples(h, &rs, vx.data(), nullptr, vth.data(), n, &ga, cl.data(), &b));
        const double al = us_since(t0);
        if (c >= 3) { t4.push_back(a4); t1.push_back(a1); tl.push_back(al); }
      }
      CHECK(h, sfw_score_sequences(h, &rs, cx.data(), nullptr, cth.data(), n, K, knot_step, &ga, cc.data(), &b));
      int64_t changed = 0;
      for (int32_t t = 0; t < n; ++t) {
        if (!same_bits(c1[t], cl[t]) || !same_bits(cc[t], cl[t])) ++mismatches;
        changed += same_bits(c4[t], cl[t]) ? 0 : 1;
      }
      std::printf("%8d %8d | %12.1f %12.1f %12.1f | %.3f   (%lld of %d costs differ from the held command's)\n", people, n, median(t4),
                  median(t1), median(tl), median(t4) / median(tl), static_cast<long long>(changed), n);
      std::fflush(stdout);
    }
    sfw_destroy(h);
  }
  std::printf("%s\n", mismatches ? "COST MISMATCH" : "K = 1 and constant K = 4 sequences equal the list, bit for bit");
  return mismatches ? 2 : 0;
}
