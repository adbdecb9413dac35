// The host engine's wh_adam_step (csrc/host_engine.cpp, csrc/sac_formula.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer: the 24 segments of tests/adam_cases.py (counts 0 .. 300,000) in one call at
// step counts 1, 2 and 1000, every tensor a heap buffer of exactly its count -- so any read or write past
// one is reported -- and the results checked against a double-precision evaluation of the header's formula
// within the bounds of tests/adam_cases.py.  Built and run by tests/test_asan_adam.py; prints
// "ASAN ADAM OK" on a clean run.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

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

const int64_t kCounts[WH_ADAM_MAX_SEGS] = {0,    1,    3, 4, 5,   4095, 4096, 4097, 300000, 2049, 2047, 2048,
                                           7,    0,    513, 9, 1025, 64,   255,  257,  2,      6,    8191, 1};

void run(int t, std::mt19937& rng) {
  std::normal_distribution<float> nd(0.0f, 1.0f);
  std::vector<std::vector<float>> p(WH_ADAM_MAX_SEGS), m(WH_ADAM_MAX_SEGS), v(WH_ADAM_MAX_SEGS), g(WH_ADAM_MAX_SEGS);
  wh_adam_seg segs[WH_ADAM_MAX_SEGS];
  for (int s = 0; s < WH_ADAM_MAX_SEGS; ++s) {
    const size_t c = (size_t)kCounts[s];
    for (auto* a : {&p[s], &m[s], &v[s], &g[s]}) {
      a->resize(c);
      for (auto& x : *a) x = nd(rng);
    }
    for (auto& x : v[s]) x = 0.01f * x * x;
    const float planted[4] = {0.0f, -0.0f, 1e-30f, 1e30f};
    for (size_t i = 0; i < c && i < 4; ++i) g[s][i] = planted[i];
    if (c) v[s][0] = 0.0f;
    segs[s] = wh_adam_seg{p[s].data(), m[s].data(), v[s].data(), g[s].data(), (int64_t)c};
  }
  const auto p0 = p, m0 = m, v0 = v;
  const double lr = 3e-4, b1 = 0.9, b2 = 0.999;
  wh_adam_hyper h{(float)b1, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), 1e-8f, (float)(lr / (1.0 - pow(b1, t))),
                  (float)sqrt(1.0 - pow(b2, t))};
  EXPECT(wh_adam_step(WH_ADAM_MAX_SEGS, segs, &h, nullptr) == WH_OK);
  const double e24 = ldexp(1.0, -24);
  for (int s = 0; s < WH_ADAM_MAX_SEGS; ++s)
    for (size_t i = 0; i < (size_t)kCounts[s]; ++i) {
      const double gg = g[s][i], sq = ((double)h.omb2 * gg) * gg;
      if (sq >= 3.4e38) {   // the planted 1e30: v' overflows f32, the step is 0
        EXPECT(isinf(v[s][i]) && p[s][i] == p0[s][i]);
        continue;
      }
      const double m1 = (double)h.beta1 * m0[s][i] + (double)h.omb1 * gg, v1 = (double)h.beta2 * v0[s][i] + sq;
      const double denom = sqrt(v1) / h.sqrt_bc2 + h.eps, D = h.step_size * (m1 / denom);
      const double A = fabs((double)h.beta1 * m0[s][i]) + fabs((double)h.omb1 * gg);
      EXPECT(fabs(m[s][i] - m1) <= 3 * e24 * A);
      EXPECT(fabs(v[s][i] - v1) <= 4 * e24 * v1);
      EXPECT(fabs(p[s][i] - (p0[s][i] - D)) <= h.step_size / denom * 3 * e24 * A + 8 * e24 * fabs(D) + e24 * fabs(p0[s][i]));
    }
}

}  // namespace

int main() {
  std::mt19937 rng(99);
  for (int t : {1, 2, 1000}) run(t, rng);
  wh_adam_hyper h{};
  wh_adam_seg bad{nullptr, nullptr, nullptr, nullptr, 3}, empty{nullptr, nullptr, nullptr, nullptr, 0};
  EXPECT(wh_adam_step(0, nullptr, &h, nullptr) == WH_OK);
  EXPECT(wh_adam_step(1, &empty, &h, nullptr) == WH_OK);
  EXPECT(wh_adam_step(1, &bad, &h, nullptr) == WH_EINVAL);
  EXPECT(wh_adam_step(1, nullptr, &h, nullptr) == WH_EINVAL);
  EXPECT(wh_adam_step(1, &empty, nullptr, nullptr) == WH_EINVAL);
  EXPECT(wh_adam_step(25, &empty, &h, nullptr) == WH_EINVAL);
  EXPECT(wh_adam_step(-1, &empty, &h, nullptr) == WH_EINVAL);
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("ASAN ADAM OK\n");
  return 0;
}
