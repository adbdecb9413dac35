// The host engine's wh_sac_td (csrc/host_engine.cpp, csrc/sac_formula.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer: every agent count and batch size of tests/sac_cases.py with every
// option case (twin / single / no Q networks, twin / single target, n given or NULL, dones masked or
// not, alpha 0 and 0.2, stray actions, n of -1, 0, partial and NA), each array a heap buffer of
// exactly the stated size -- so any read or write past one is reported -- and the results checked
// against a double-precision evaluation of the header's formula.  Built and run by
// tests/test_asan_sac.py; prints "ASAN SAC OK" on a clean run.
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
  bool twin_t;
  int nq;   // Q networks: 2, 1, or 0 (targets only)
  bool use_n;
  int mask;
  float alpha;
};

const Case kCases[] = {{true, 2, true, 0, 0.2f},  {true, 2, false, 1, 0.0f}, {false, 1, true, 1, 0.2f},
                       {true, 1, true, 0, 0.2f},  {true, 0, true, 0, 0.2f},  {false, 0, false, 1, 0.2f}};

void run(int64_t M, int NA, const Case& c, std::mt19937& rng) {
  const size_t rows = (size_t)M * NA;
  std::uniform_real_distribution<float> ul(-4.0f, 4.0f), uq(-10.0f, 10.0f);
  const float rw[4] = {-1.0f, 0.0f, 1.0f, 10.0f};
  std::vector<float> pi(rows * 9), q1t(rows * 9), q2t(rows * 9), q1(rows * 9), q2(rows * 9), rewards(rows);
  std::vector<int32_t> actions(rows), n((size_t)M);
  std::vector<uint8_t> dones((size_t)M);
  for (auto& v : pi) v = ul(rng);
  for (auto* a : {&q1t, &q2t, &q1, &q2})
    for (auto& v : *a) v = uq(rng);
  for (size_t r = 0; r < rows; ++r) {
    rewards[r] = rw[rng() % 4];
    actions[r] = (int32_t)(rng() % 9);
  }
  actions[0] = -3;
  actions[rows - 1] = 9;
  const int nv[5] = {-1, 0, std::max(1, NA / 2), std::max(1, NA - 1), NA};
  for (int64_t m = 0; m < M; ++m) {
    n[(size_t)m] = m == 0 ? NA : nv[rng() % 5];
    dones[(size_t)m] = rng() % 3 == 0;
  }
  std::vector<float> y(rows, -7.0f), td_rows(rows, -7.0f), td((size_t)M, -7.0f);
  wh_sac_td_args a{};
  a.pi_next = pi.data();
  a.q1t_next = q1t.data();
  a.q2t_next = c.twin_t ? q2t.data() : nullptr;
  a.q1 = c.nq >= 1 ? q1.data() : nullptr;
  a.q2 = c.nq >= 2 ? q2.data() : nullptr;
  a.actions = actions.data();
  a.rewards = rewards.data();
  a.dones = c.mask ? dones.data() : nullptr;
  a.n = c.use_n ? n.data() : nullptr;
  a.alpha = c.alpha;
  a.discount = 0.97f;
  a.mask_dones = c.mask;
  a.y = y.data();
  a.td_rows = c.nq ? td_rows.data() : nullptr;
  a.td = c.nq ? td.data() : nullptr;
  EXPECT(wh_sac_td(M, NA, &a, nullptr) == WH_OK);
  const double S = 10.0 + 0.97 * (10.0 + c.alpha * (8.0 + log(9.0)));
  const double by = 64.0 * ldexp(1.0, -24) * S, btd = 2.0 * (64 + NA) * ldexp(1.0, -24) * (S + 10.0);
  for (int64_t m = 0; m < M; ++m) {
    const int live = c.use_n ? std::min(std::max(n[(size_t)m], 0), NA) : NA;
    double sum = 0.0;
    for (int i = 0; i < NA; ++i) {
      const size_t r = (size_t)m * NA + i, e = r * 9;
      double want_y = 0.0, want_td = 0.0;
      if (i < live) {
        double zmax = pi[e], s = 0.0, v = 0.0;
        for (int o = 1; o < 9; ++o) zmax = std::max(zmax, (double)pi[e + o]);
        for (int o = 0; o < 9; ++o) s += exp(pi[e + o] - zmax);
        const double lse = zmax + log(s);
        for (int o = 0; o < 9; ++o) {
          const double logp = pi[e + o] - lse;
          const double q = c.twin_t ? std::min((double)q1t[e + o], (double)q2t[e + o]) : (double)q1t[e + o];
          v += exp(logp) * (q - (double)c.alpha * logp);
        }
        want_y = rewards[r] + (double)0.97f * ((c.mask && dones[(size_t)m]) ? 0.0 : v);
        if (c.nq) {
          const int act = (actions[r] >= 0 && actions[r] < 9) ? actions[r] : 4;
          want_td = fabs(q1[e + act] - want_y);
          if (c.nq == 2) want_td = 0.5 * (want_td + fabs(q2[e + act] - want_y));
        }
        EXPECT(fabs(y[r] - want_y) <= by);
        if (c.nq) EXPECT(fabs(td_rows[r] - want_td) <= by);
      } else {
        EXPECT(y[r] == 0.0f);
        if (c.nq) EXPECT(td_rows[r] == 0.0f);
      }
      sum += want_td;
    }
    if (c.nq) {
      if (live > 0) EXPECT(fabs(td[(size_t)m] - sum / live) <= btd);
      else EXPECT(td[(size_t)m] == 0.0f);
    }
  }
}

}  // namespace

int main() {
  std::mt19937 rng(12345);
  for (int NA : {1, 4, 9, 16})
    for (int64_t M : {1, 65, 300})
      for (const Case& c : kCases) run(M, NA, c, rng);
  // refusals and the empty batch touch nothing
  wh_sac_td_args a{};
  EXPECT(wh_sac_td(0, 4, &a, nullptr) == WH_OK);
  EXPECT(wh_sac_td(3, 4, &a, nullptr) == WH_EINVAL);
  EXPECT(wh_sac_td(3, 4, nullptr, nullptr) == WH_EINVAL);
  EXPECT(wh_sac_td(-1, 4, &a, nullptr) == WH_EINVAL);
  EXPECT(wh_sac_td(3, 17, &a, nullptr) == WH_EINVAL);
  EXPECT(wh_mlp_pack_device(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == WH_ENOTSUP);
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("ASAN SAC OK\n");
  return 0;
}
