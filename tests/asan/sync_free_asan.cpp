// The host engine's wh_sac_td_la and wh_adam_step_clock (csrc/host_engine.cpp, csrc/sac_formula.h) under
// AddressSanitizer + UndefinedBehaviorSanitizer.  Every array is a heap buffer of exactly its stated size
// -- log_alpha one float, the clock sizeof(wh_adam_clock) bytes -- so any read or write past one is
// reported.  wh_sac_td_la at NA in {1, 4, 8, 16} and M in {1, 33} must give wh_sac_td's outputs at
// alpha = expf(log_alpha) bit for bit; three chained wh_adam_step_clock calls over the 24 segments of
// tests/adam_cases.py must leave the tensors wh_adam_step leaves with the header's table of the same step,
// bit for bit, and the clock at t = 3.  Built and run by tests/test_asan_sync_free.py; prints
// "ASAN SYNC FREE OK" on a clean run.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
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

template <class T>
bool same_bits(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

void run_td(int NA, int64_t M, float la, std::mt19937& rng) {
  std::uniform_real_distribution<float> logit(-4.0f, 4.0f), qv(-10.0f, 10.0f);
  std::uniform_int_distribution<int> act(-1, 9), cnt(-1, NA);
  const size_t rows = (size_t)(M * NA);
  std::vector<float> pi(rows * 9), q1t(rows * 9), q2t(rows * 9), q1(rows * 9), q2(rows * 9), rew(rows);
  std::vector<int32_t> actions(rows), n((size_t)M);
  std::vector<uint8_t> dones((size_t)M);
  for (auto& x : pi) x = logit(rng);
  for (auto* a : {&q1t, &q2t, &q1, &q2})
    for (auto& x : *a) x = qv(rng);
  for (auto& x : rew) x = (float)(act(rng) % 3);
  for (auto& x : actions) x = act(rng);
  for (auto& x : n) x = cnt(rng);
  for (auto& x : dones) x = (uint8_t)(act(rng) & 1);
  n[0] = NA;
  std::unique_ptr<float> log_alpha(new float(la));
  std::vector<float> y(rows), tdr(rows), td((size_t)M), y2(rows), tdr2(rows), td2((size_t)M);
  wh_sac_td_args a{pi.data(), q1t.data(), q2t.data(), q1.data(), q2.data(), actions.data(), rew.data(), dones.data(),
                   n.data(), NAN, 0.97f, 1, y.data(), tdr.data(), td.data()};
  EXPECT(wh_sac_td_la(M, NA, &a, log_alpha.get(), nullptr) == WH_OK);
  wh_sac_td_args b = a;
  b.alpha = expf(la);
  b.y = y2.data(), b.td_rows = tdr2.data(), b.td = td2.data();
  EXPECT(wh_sac_td(M, NA, &b, nullptr) == WH_OK);
  EXPECT(same_bits(y, y2) && same_bits(tdr, tdr2) && same_bits(td, td2));
  EXPECT(*log_alpha == la);
  // targets only, no twin, no n, no mask: the optional arrays absent
  wh_sac_td_args c{pi.data(), q1t.data(), nullptr, nullptr, nullptr, actions.data(), rew.data(), nullptr, nullptr,
                   NAN, 0.97f, 0, y.data(), nullptr, nullptr};
  EXPECT(wh_sac_td_la(M, NA, &c, log_alpha.get(), nullptr) == WH_OK);
  c.alpha = expf(la);
  c.y = y2.data();
  EXPECT(wh_sac_td(M, NA, &c, nullptr) == WH_OK);
  EXPECT(same_bits(y, y2));
}

const int64_t kCounts[WH_ADAM_MAX_SEGS] = {0,    1,    3, 4, 5,   4095, 4096, 4097, 300000, 2049, 2047, 2048,
                                           7,    0,    513, 9, 1025, 64,   255,  257,  2,      6,    8191, 1};

void run_clock(std::mt19937& rng) {
  std::normal_distribution<float> nd(0.0f, 1.0f);
  std::vector<std::vector<float>> p(WH_ADAM_MAX_SEGS), m(WH_ADAM_MAX_SEGS), v(WH_ADAM_MAX_SEGS), g(WH_ADAM_MAX_SEGS);
  for (int s = 0; s < WH_ADAM_MAX_SEGS; ++s) {
    for (auto* a : {&p[s], &m[s], &v[s], &g[s]}) {
      a->resize((size_t)kCounts[s]);
      for (auto& x : *a) x = nd(rng);
    }
    for (auto& x : v[s]) x = 0.01f * x * x;
  }
  auto p2 = p, m2 = m, v2 = v;
  wh_adam_seg segs[WH_ADAM_MAX_SEGS], segs2[WH_ADAM_MAX_SEGS];
  for (int s = 0; s < WH_ADAM_MAX_SEGS; ++s) {
    segs[s] = wh_adam_seg{p[s].data(), m[s].data(), v[s].data(), g[s].data(), kCounts[s]};
    segs2[s] = wh_adam_seg{p2[s].data(), m2[s].data(), v2[s].data(), g[s].data(), kCounts[s]};
  }
  const double lr = 3e-4, b1 = 0.9, b2 = 0.999, eps = 1e-8;
  std::unique_ptr<wh_adam_clock> clock(new wh_adam_clock{0, 1.0, 1.0, {}});
  double b1t = 1.0, b2t = 1.0;
  for (int t = 1; t <= 3; ++t) {
    for (auto& a : g)
      for (auto& x : a) x = nd(rng);
    EXPECT(wh_adam_step_clock(WH_ADAM_MAX_SEGS, segs, clock.get(), lr, b1, b2, eps, nullptr) == WH_OK);
    b1t *= b1, b2t *= b2;
    const wh_adam_hyper h{(float)b1, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)eps,
                          (float)(lr / (1.0 - b1t)), (float)sqrt(1.0 - b2t)};
    EXPECT(clock->t == t && clock->beta1_t == b1t && clock->beta2_t == b2t);
    EXPECT(memcmp(&clock->h, &h, sizeof h) == 0);
    EXPECT(wh_adam_step(WH_ADAM_MAX_SEGS, segs2, &h, nullptr) == WH_OK);
    for (int s = 0; s < WH_ADAM_MAX_SEGS; ++s) EXPECT(same_bits(p[s], p2[s]) && same_bits(m[s], m2[s]) && same_bits(v[s], v2[s]));
  }
  // no tensors: the clock still ticks; refused calls leave it alone
  wh_adam_seg bad{nullptr, nullptr, nullptr, nullptr, 3}, empty{nullptr, nullptr, nullptr, nullptr, 0};
  EXPECT(wh_adam_step_clock(0, nullptr, clock.get(), lr, b1, b2, eps, nullptr) == WH_OK && clock->t == 4);
  EXPECT(wh_adam_step_clock(1, &empty, clock.get(), lr, b1, b2, eps, nullptr) == WH_OK && clock->t == 5);
  EXPECT(wh_adam_step_clock(1, &bad, clock.get(), lr, b1, b2, eps, nullptr) == WH_EINVAL);
  EXPECT(wh_adam_step_clock(1, nullptr, clock.get(), lr, b1, b2, eps, nullptr) == WH_EINVAL);
  EXPECT(wh_adam_step_clock(1, &empty, nullptr, lr, b1, b2, eps, nullptr) == WH_EINVAL);
  EXPECT(wh_adam_step_clock(25, &empty, clock.get(), lr, b1, b2, eps, nullptr) == WH_EINVAL);
  EXPECT(wh_adam_step_clock(-1, &empty, clock.get(), lr, b1, b2, eps, nullptr) == WH_EINVAL);
  EXPECT(wh_adam_step_clock(1, &empty, reinterpret_cast<wh_adam_clock*>(reinterpret_cast<char*>(clock.get()) + 4), lr, b1,
                            b2, eps, nullptr) == WH_EINVAL);
  EXPECT(clock->t == 5);
}

}  // namespace

int main() {
  std::mt19937 rng(7);
  for (int NA : {1, 4, 8, 16})
    for (int64_t M : {(int64_t)1, (int64_t)33})
      for (float la : {0.0f, -1.609438f, -3.0f, 1.0f}) run_td(NA, M, la, rng);
  run_clock(rng);
  float one = 0.0f;
  wh_sac_td_args a{};
  EXPECT(wh_sac_td_la(0, 4, &a, nullptr, nullptr) == WH_OK);
  EXPECT(wh_sac_td_la(0, 4, nullptr, &one, nullptr) == WH_EINVAL);
  float buf[36] = {};
  int32_t act[4] = {};
  wh_sac_td_args ok{buf, buf, nullptr, nullptr, nullptr, act, buf, nullptr, nullptr, 0.2f, 0.9f, 0, buf, nullptr, nullptr};
  EXPECT(wh_sac_td_la(1, 4, &ok, nullptr, nullptr) == WH_EINVAL);
  EXPECT(wh_sac_td_la(1, 17, &ok, &one, nullptr) == WH_EINVAL);
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("ASAN SYNC FREE OK\n");
  return 0;
}
