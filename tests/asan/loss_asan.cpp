// The host engine's wh_sac_loss (csrc/host_engine.cpp, csrc/sac_formula.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer: every agent count and batch size of tests/sac_cases.py with the option
// cases of tests/loss_cases.py (twin / single, n given or NULL, weights given or NULL, some outputs NULL,
// stray actions, n of -1, 0, partial and NA), each array a heap buffer of exactly the stated size -- so
// any read or write past one is reported -- and the results checked against a double-precision
// evaluation of the header's formula within the bounds of tests/loss_cases.py.  Built and run by
// tests/test_asan_loss.py; prints "ASAN LOSS OK" on a clean run.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

#include "warehouse_amd.h"

namespace {

int fails = 0;
#define EXPECT(c)                                                  \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                     \
    }                                                              \
  } while (0)

struct Case {
  bool twin, use_n, use_w;
  bool dpi, dq1, dq2;   // which gradient outputs are given
};

const Case kCases[] = {{true, true, true, true, true, true},     {false, false, false, true, true, false},
                       {true, true, false, false, true, false},  {true, false, true, true, false, true},
                       {false, true, true, false, false, false}};

void run(int64_t M, int NA, const Case& c, std::mt19937& rng) {
  const size_t rows = (size_t)M * NA;
  std::uniform_real_distribution<float> ul(-4.0f, 4.0f), uq(-10.0f, 10.0f), uy(-20.0f, 20.0f), uw(0.25f, 1.0f);
  std::vector<float> pi(rows * 9), q1(rows * 9), q2(rows * 9), y(rows), w((size_t)M), la(1, logf(0.2f));
  std::vector<int32_t> actions(rows), n((size_t)M);
  for (auto& v : pi) v = ul(rng);
  for (auto* a : {&q1, &q2})
    for (auto& v : *a) v = uq(rng);
  for (size_t r = 0; r < rows; ++r) {
    y[r] = uy(rng);
    actions[r] = (int32_t)(rng() % 9);
  }
  actions[0] = -3;
  actions[rows - 1] = 9;
  const int nv[5] = {-1, 0, std::max(1, NA / 2), std::max(1, NA - 1), NA};
  for (int64_t m = 0; m < M; ++m) {
    n[(size_t)m] = m == 0 ? NA : nv[rng() % 5];
    w[(size_t)m] = uw(rng);
  }
  int64_t work_bytes = 0;
  EXPECT(wh_sac_loss_query(M, NA, &work_bytes) == WH_OK && work_bytes >= 32 && work_bytes % 16 == 0);
  std::vector<float> dpi(rows * 9, -7.0f), dq1(rows * 9, -7.0f), dq2(rows * 9, -7.0f), stats(6, -7.0f);
  void* work = aligned_alloc(16, (size_t)work_bytes);
  const float te = 0.935f, scale = 1.0f / (float)rows;
  wh_sac_loss_args a{};
  a.pi = pi.data();
  a.q1 = q1.data();
  a.q2 = c.twin ? q2.data() : nullptr;
  a.y = y.data();
  a.actions = actions.data();
  a.n = c.use_n ? n.data() : nullptr;
  a.weights = c.use_w ? w.data() : nullptr;
  a.log_alpha = la.data();
  a.target_entropy = te;
  a.scale = scale;
  a.dpi = c.dpi ? dpi.data() : nullptr;
  a.dq1 = c.dq1 ? dq1.data() : nullptr;
  a.dq2 = c.dq2 ? dq2.data() : nullptr;
  a.stats = stats.data();
  a.work = work;
  EXPECT(wh_sac_loss(M, NA, &a, nullptr) == WH_OK);
  free(work);
  const double alpha = exp((double)la[0]), eps24 = ldexp(1.0, -24);
  const double G = alpha * (8.0 + log(9.0)) + 10.0, E = 8.0 + log(9.0) + te, C = 0.5 * 30.0 * 30.0;
  const double bdpi = 64 * eps24 * 2 * G * scale, bdq = 8 * eps24 * 30.0 * scale;
  const int spw = 256 / NA;
  const double depth = (64 + 256 + (double)((M + spw - 1) / spw)) * eps24 * scale * (double)rows;
  double s1 = 0, s2 = 0, sf = 0, st = 0, livecount = 0;
  for (int64_t m = 0; m < M; ++m) {
    const int live = c.use_n ? std::min(std::max(n[(size_t)m], 0), NA) : NA;
    const double wm = c.use_w ? w[(size_t)m] : 1.0;
    for (int i = 0; i < NA; ++i) {
      const size_t r = (size_t)m * NA + i, e = r * 9;
      if (i >= live) {
        for (int o = 0; o < 9; ++o) {
          if (c.dpi) EXPECT(dpi[e + o] == 0.0f);
          if (c.dq1) EXPECT(dq1[e + o] == 0.0f);
          if (c.dq2) EXPECT(dq2[e + o] == 0.0f);
        }
        continue;
      }
      double zmax = pi[e], s = 0.0, f = 0.0, t = 0.0, p[9], g[9];
      for (int o = 1; o < 9; ++o) zmax = std::max(zmax, (double)pi[e + o]);
      for (int o = 0; o < 9; ++o) s += exp(pi[e + o] - zmax);
      const double lse = zmax + log(s);
      for (int o = 0; o < 9; ++o) {
        const double logp = pi[e + o] - lse;
        p[o] = exp(logp);
        const double qm = c.twin ? std::min((double)q1[e + o], (double)q2[e + o]) : (double)q1[e + o];
        g[o] = alpha * logp - qm;
        f += p[o] * g[o];
        t += p[o] * (logp + te);
      }
      const int act = (actions[r] >= 0 && actions[r] < 9) ? actions[r] : 4;
      const double e1 = q1[e + act] - (double)y[r], e2 = q2[e + act] - (double)y[r];
      for (int o = 0; o < 9; ++o) {
        if (c.dpi) EXPECT(fabs(dpi[e + o] - scale * p[o] * (g[o] - f)) <= bdpi);
        if (c.dq1) EXPECT(fabs(dq1[e + o] - (o == act ? scale * wm * e1 : 0.0)) <= bdq);
        if (c.dq2) EXPECT(fabs(dq2[e + o] - (o == act ? scale * wm * e2 : 0.0)) <= bdq);
      }
      s1 += 0.5 * wm * e1 * e1;
      if (c.twin) s2 += 0.5 * wm * e2 * e2;
      sf += f;
      st += t;
      livecount += 1;
    }
  }
  const double T = scale * st;
  EXPECT(fabs(stats[0] - scale * s1) <= depth * C);
  EXPECT(fabs(stats[1] - scale * s2) <= depth * C);
  EXPECT(fabs(stats[2] - scale * sf) <= depth * G);
  EXPECT(fabs(stats[3] - (-(double)la[0]) * T) <= depth * E * fabs(la[0]) + fabs(T) * ldexp(1.0, -22));
  EXPECT(fabs(stats[4] - (-T)) <= depth * E);
  EXPECT(stats[5] == (float)livecount);
}

}  // namespace

int main() {
  std::mt19937 rng(4321);
  for (int NA : {1, 2, 3, 4, 5, 8, 9, 10, 11, 16})
    for (int64_t M : {1, 65, 300})
      for (const Case& c : kCases) run(M, NA, c, rng);
  // refusals and the empty batch touch nothing
  wh_sac_loss_args a{};
  EXPECT(wh_sac_loss(0, 4, &a, nullptr) == WH_OK);
  EXPECT(wh_sac_loss(3, 4, &a, nullptr) == WH_EINVAL);
  EXPECT(wh_sac_loss(3, 4, nullptr, nullptr) == WH_EINVAL);
  EXPECT(wh_sac_loss(-1, 4, &a, nullptr) == WH_EINVAL);
  EXPECT(wh_sac_loss(3, 17, &a, nullptr) == WH_EINVAL);
  EXPECT(wh_sac_loss_query(3, 0, nullptr) == WH_EINVAL);
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("ASAN LOSS OK\n");
  return 0;
}
