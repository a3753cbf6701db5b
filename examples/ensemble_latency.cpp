// ensemble_latency.cpp — one robot's grid under M crowd hypotheses (naive goals at other horizons and headings) scored three
// ways through the C ABI; medians of the wall-clock of one call:
//   (a) M blocking sfw_score_grid calls on one handle (terms capture on, sfw_grid_terms for the social work), the
//       aggregation and the selection on the host;
//   (b) sfw_ensemble_score_grid, split into stage / enqueue / wait + copies (sfw_ensemble_last_us);
//   (c) sfw_ensemble_aggregate alone (another mode on the same launch).
// Every (b) selection is checked against (a) field by field.
//
//   build: make -C social_force_window_planner_amd/csrc ensemblelatency
//   run:   build/ensemble_latency [cycles]
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

// hypothesis m: naive goal time 1 + m % 4 s, heading turned by 0.3 * (m / 4) rad, alternating sign (as naive_goal_hypotheses)
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
  return h;
}

// the reference's selection (src/sfw_planner.cpp:394-414) over a cost vector
static sfw_best select_host(const std::vector<double> &c, const double *lin, const double *ang, int nw) {
  sfw_best b{-1, -1.0, 0.0, 0.0, 0.0, 0};
  double bc = 10000.0, bl = 0.0, ba = 0.0;
  for (size_t t = 0; t < c.size(); ++t) {
    if (!(c[t] >= 0.0)) continue;
    ++b.n_valid;
    const double l = lin[t / nw], a = ang[t % nw];
    const bool better = c[t] < bc || (c[t] == bc && (l > bl || (l == bl && std::fabs(a) <= std::fabs(ba))));
    if (better) { bc = c[t]; bl = l; ba = a; b.index = static_cast<int64_t>(t); }
  }
  if (b.index >= 0) { b.cost = bc; b.vx = bl; b.vtheta = ba; }
  return b;
}

int main(int argc, char **argv) {
  const int cycles = argc > 1 ? std::atoi(argv[1]) : 30;
  std::printf("one robot, M crowd hypotheses, medians of %d calls (us): (a) M x sfw_score_grid + terms + host aggregation, "
              "(b) sfw_ensemble_score_grid [stage + enqueue + wait/copies], (c) sfw_ensemble_aggregate\n", cycles);
  struct grid_case { int nv, nw, n_people; unsigned cells; std::vector<int> Ms; int cycles; };
  const std::vector<grid_case> cases = {{5, 9, 5, 200, {1, 2, 4, 8, 16}, cycles},
                                        {5, 9, 20, 200, {1, 2, 4, 8, 16}, cycles},
                                        {256, 256, 50, 500, {1, 4}, std::max(3, cycles / 3)}};
  int mismatches = 0;
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
    const int64_t T = static_cast<int64_t>(gc.nv) * gc.nw;
    const world w = make_world(gc.n_people, gc.cells);
    const double origin = -(gc.cells * 0.05) / 2.0;
    sfw_params p;
    sfw_params_default(&p);
    const int S = static_cast<int>(p.sim_time / p.sim_granularity + 0.5);
    const sfw_robot_state rs{0.0, 0.0, 0.0, 0.3, 0.0, 0.0};
    const sfw_goal_args ga{1.0, 0.0, 1.0, 2.0, 0.5};
    for (int M : gc.Ms) {
      std::vector<std::vector<sfw_agent>> hyps;
      for (int m = 0; m < M; ++m) hyps.push_back(hypothesis(w.ag, m));
      // (a)
      sfw_handle one = nullptr;
      if (sfw_create(&p, 0, &one) != SFW_OK) {
        std::fprintf(stderr, "sfw_create failed (no HIP device?)\n");
        return 1;
      }
      if (sfw_set_costmap(one, w.cells.data(), w.n, w.n, origin, origin, 0.05) != SFW_OK || sfw_set_footprint(one, w.fp.data(), 16) != SFW_OK ||
          sfw_set_terms_capture(one, 1) != SFW_OK)
        return 1;
      std::vector<double> costs(static_cast<size_t>(T)), terms(static_cast<size_t>(T) * SFW_N_TERMS), t0terms, acc(static_cast<size_t>(T));
      std::vector<int32_t> rej(static_cast<size_t>(T));
      sfw_best host_best{};
      std::vector<double> ta, tb, tc, u0s, u1s, u2s;
      for (int c = 0; c < gc.cycles + 3; ++c) {
        const auto t0 = clk::now();
        std::fill(rej.begin(), rej.end(), 0);
        std::fill(acc.begin(), acc.end(), 0.0);
        for (int m = 0; m < M; ++m) {
          if (sfw_set_agents(one, hyps[m].data(), static_cast<int>(hyps[m].size()), nullptr, 0) != SFW_OK ||
              sfw_score_grid(one, &rs, lin.data(), gc.nv, ang.data(), gc.nw, &ga, costs.data(), nullptr) != SFW_OK ||
              sfw_grid_terms(one, 0, T, terms.data()) != SFW_OK)
            return 1;
          if (m == 0) t0terms = terms;
          for (int64_t t = 0; t < T; ++t) {
            rej[t] += costs[t] == SFW_COST_INVALID ? 1 : 0;
            acc[t] = acc[t] + (1.0 / M) * terms[t * SFW_N_TERMS + SFW_TERM_SOCIAL];  // (SFW_ENSEMBLE_MEAN, p = 1 / M)
          }
        }
        std::vector<double> ec(static_cast<size_t>(T));
        for (int64_t t = 0; t < T; ++t) {
          const double *q = &t0terms[t * SFW_N_TERMS];
          if (q[SFW_TERM_DISTANCE] == SFW_COST_SKIPPED) ec[t] = SFW_COST_SKIPPED;
          else if (rej[t] > 0) ec[t] = SFW_COST_INVALID;
          else {
            const double base = p.vel_weight * q[SFW_TERM_VEL] + p.distance_weight * q[SFW_TERM_DISTANCE] + p.angle_weight * q[SFW_TERM_ANGLE];
            ec[t] = std::fma(p.social_weight, acc[t], base + p.costmap_weight * q[SFW_TERM_COSTMAP]);
          }
        }
        host_best = select_host(ec, lin.data(), ang.data(), gc.nw);
        if (c >= 3) ta.push_back(us_since(t0));
      }
      sfw_destroy(one);
      // (b), (c)
      sfw_ensemble e = nullptr;
      if (sfw_ensemble_create(&p, 0, M, &e) != SFW_OK || sfw_ensemble_set_costmap(e, w.cells.data(), w.n, w.n, origin, origin, 0.05) != SFW_OK ||
          sfw_ensemble_set_footprint(e, w.fp.data(), 16) != SFW_OK)
        return 1;
      for (int m = 0; m < M; ++m)
        if (sfw_ensemble_set_hypothesis(e, m, hyps[m].data(), static_cast<int>(hyps[m].size()), nullptr, 0) != SFW_OK) return 1;
      sfw_best eb{}, ab{};
      for (int c = 0; c < gc.cycles + 3; ++c) {
        auto t0 = clk::now();
        if (sfw_ensemble_score_grid(e, &rs, lin.data(), gc.nv, ang.data(), gc.nw, &ga, SFW_ENSEMBLE_MEAN, nullptr, costs.data(),
                                    rej.data(), &eb) != SFW_OK) {
          std::fprintf(stderr, "ensemble: %s\n", sfw_ensemble_last_error(e));
          return 1;
        }
        const double t = us_since(t0);
        double u0 = 0, u1 = 0, u2 = 0;
        sfw_ensemble_last_us(e, 0, &u0);
        sfw_ensemble_last_us(e, 1, &u1);
        sfw_ensemble_last_us(e, 2, &u2);
        t0 = clk::now();
        if (sfw_ensemble_aggregate(e, SFW_ENSEMBLE_MAX, nullptr, costs.data(), rej.data(), &ab) != SFW_OK) return 1;
        const double ta2 = us_since(t0);
        if (c >= 3) { tb.push_back(t); u0s.push_back(u0); u1s.push_back(u1); u2s.push_back(u2); tc.push_back(ta2); }
      }
      sfw_ensemble_destroy(e);
      const bool same = eb.index == host_best.index && eb.cost == host_best.cost && eb.vx == host_best.vx &&
                        eb.vy == host_best.vy && eb.vtheta == host_best.vtheta && eb.n_valid == host_best.n_valid;
      mismatches += same ? 0 : 1;
      std::printf("grid %3dx%-3d N=%2d S=%2d M=%2d: (a) %9.1f  (b) %9.1f [%7.1f + %7.1f + %7.1f]  (c) %7.1f  best %lld (%s) max-best %lld\n",
                  gc.nv, gc.nw, gc.n_people, S, M, median(ta), median(tb), median(u0s), median(u1s), median(u2s), median(tc),
                  static_cast<long long>(eb.index), same ? "= (a)" : "DIFFERS from (a)", static_cast<long long>(ab.index));
      std::fflush(stdout);
    }
  }
  std::printf("%s\n", mismatches ? "SELECTION MISMATCH" : "every (b) selection equals (a)");
  return mismatches ? 2 : 0;
}
