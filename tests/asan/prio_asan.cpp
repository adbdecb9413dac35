// The host engine's replay priority tree (csrc/host_engine.cpp: wh_replay_prio_*) under
// AddressSanitizer + UndefinedBehaviorSanitizer: trees of 1 .. 6 levels (up to 1,048,577 leaves) with buffers of exactly the
// sizes wh_replay_prio_query states, fills over every kind of range, updates with duplicate and
// invalid indices and the quantisation's edge values, samples from injected and philox draws, the
// largest sums, the empty tree and the refusals -- so any read or write past a buffer, any signed
// overflow or bad float conversion is reported.  Built and run by tests/test_asan_prio.py; prints
// "ASAN PRIO OK" on a clean run.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <limits>
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

struct Tree {
  std::vector<uint32_t> leaf;
  std::vector<uint64_t> node;
  uint32_t max_q = WH_PRIO_ONE;
  int32_t levels = 0;
  wh_replay_prio t{};
  explicit Tree(int64_t count) {
    int64_t lw = 0, nw = 0;
    EXPECT(wh_replay_prio_query(count, &lw, &nw, &levels) == WH_OK);
    leaf.assign((size_t)lw, 0u);
    node.assign((size_t)nw, 0ull);
    t = wh_replay_prio{leaf.data(), node.data(), &max_q, count};
  }
  // every sum recomputed from the level below; the root is the last level's entry 0
  uint64_t check() {
    std::vector<uint64_t> cur(leaf.begin(), leaf.end());
    size_t off = 0;
    for (int k = 1; k <= levels; ++k) {
      const size_t n = cur.size() / 16, padded = (n + 15) / 16 * 16;
      std::vector<uint64_t> next(padded, 0ull);
      for (size_t j = 0; j < cur.size(); ++j) next[j / 16] += cur[j];
      for (size_t j = 0; j < padded; ++j) EXPECT(node[off + j] == next[j]);
      off += padded;
      cur.swap(next);
    }
    EXPECT(off == node.size());
    for (size_t j = (size_t)t.count; j < leaf.size(); ++j) EXPECT(leaf[j] == 0u);
    return cur[0];
  }
};

void exercise(int64_t count, uint64_t seed) {
  Tree T(count);
  std::mt19937_64 rng(seed);
  EXPECT(T.check() == 0);
  EXPECT(wh_replay_prio_fill(&T.t, 0, count, 0, WH_PRIO_ONE, nullptr) == WH_OK);
  EXPECT(T.check() == (uint64_t)count * WH_PRIO_ONE);
  const int64_t first = count > 5 ? 5 : count - 1, n = count - first < 20 ? count - first : 20;
  EXPECT(wh_replay_prio_fill(&T.t, first, n, 0, 3u, nullptr) == WH_OK);
  EXPECT(wh_replay_prio_fill(&T.t, count - 1, 1, 0, WH_PRIO_MAX, nullptr) == WH_OK);
  EXPECT(wh_replay_prio_fill(&T.t, count, 0, 1, 0u, nullptr) == WH_OK);
  T.check();

  const float inf = std::numeric_limits<float>::infinity();
  const float edge[] = {NAN, 0.0f, -0.0f, -3.5f, 1e-9f, 9.5367431640625e-07f, 1.0f, 2047.9f, 2048.0f, 1e30f, inf, -inf, 1e-45f};
  for (int64_t M : {(int64_t)1, (int64_t)13, (int64_t)257, (int64_t)1000}) {
    std::vector<int64_t> idx((size_t)M);
    std::vector<float> p((size_t)M);
    for (int64_t m = 0; m < M; ++m) {
      idx[m] = (int64_t)(rng() % (uint64_t)count);
      p[m] = m < 13 ? edge[m] : (float)(rng() % 100000) / 2500.0f;
    }
    if (M > 4) {
      idx[1] = idx[0];
      idx[2] = -1;
      idx[3] = count;
      idx[4] = (int64_t)1 << 40;
    }
    EXPECT(wh_replay_prio_update(&T.t, M, idx.data(), p.data(), nullptr) == WH_OK);
    T.check();
  }
  EXPECT(T.max_q == WH_PRIO_MAX);
  EXPECT(wh_replay_prio_fill(&T.t, 0, count > 3 ? count / 3 : 1, 1, 0u, nullptr) == WH_OK);
  EXPECT(T.leaf[0] == WH_PRIO_MAX);
  uint64_t total = T.check();

  for (int64_t M : {(int64_t)1, (int64_t)17, (int64_t)1000}) {
    std::vector<uint64_t> u((size_t)M);
    for (auto& x : u) x = rng();
    u[0] = 0;
    u[(size_t)M - 1] = ~0ull;
    std::vector<int64_t> idx((size_t)M);
    std::vector<uint32_t> q((size_t)M);
    uint64_t tot = 0;
    EXPECT(wh_replay_prio_sample(&T.t, M, u.data(), 1, 2, idx.data(), q.data(), &tot, nullptr) == WH_OK);
    EXPECT(tot == total);
    for (int64_t m = 0; m < M; ++m) EXPECT(idx[m] >= 0 && idx[m] < count && q[m] == T.leaf[idx[m]] && q[m] > 0);
    EXPECT(wh_replay_prio_sample(&T.t, M, nullptr, seed, (uint64_t)M << 33 | 5u, idx.data(), nullptr, nullptr, nullptr) == WH_OK);
    for (int64_t m = 0; m < M; ++m) EXPECT(idx[m] >= 0 && idx[m] < count && T.leaf[idx[m]] > 0);
  }
  // the largest sums, then the empty tree
  EXPECT(wh_replay_prio_fill(&T.t, 0, count, 0, WH_PRIO_MAX, nullptr) == WH_OK);
  EXPECT(T.check() == (uint64_t)count * WH_PRIO_MAX);
  int64_t ix[2];
  uint32_t q2[2];
  const uint64_t ends[2] = {0, ~0ull};
  EXPECT(wh_replay_prio_sample(&T.t, 2, ends, 0, 0, ix, q2, &total, nullptr) == WH_OK);
  EXPECT(ix[0] == 0 && ix[1] == count - 1 && q2[0] == WH_PRIO_MAX);
  EXPECT(wh_replay_prio_fill(&T.t, 0, count, 0, 0u, nullptr) == WH_OK);
  EXPECT(T.check() == 0);
  EXPECT(wh_replay_prio_sample(&T.t, 2, ends, 0, 0, ix, q2, &total, nullptr) == WH_OK);
  EXPECT(ix[0] == -1 && ix[1] == -1 && q2[0] == 0 && q2[1] == 0 && total == 0);

  // refusals and empty calls touch nothing (NULL buffers would fault)
  wh_replay_prio bad = T.t;
  bad.leaf = nullptr;
  EXPECT(wh_replay_prio_fill(&bad, 0, 1, 0, 1u, nullptr) == WH_EINVAL);
  EXPECT(wh_replay_prio_fill(&T.t, count, 1, 0, 1u, nullptr) == WH_EINVAL);
  EXPECT(wh_replay_prio_fill(&T.t, 0, 1, 2, 1u, nullptr) == WH_EINVAL);
  EXPECT(wh_replay_prio_update(&T.t, 0, nullptr, nullptr, nullptr) == WH_OK);
  EXPECT(wh_replay_prio_update(&T.t, 1, nullptr, nullptr, nullptr) == WH_EINVAL);
  EXPECT(wh_replay_prio_sample(&T.t, 0, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr) == WH_OK);
  EXPECT(wh_replay_prio_sample(&T.t, 1, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr) == WH_EINVAL);
  EXPECT(wh_replay_prio_sample(&T.t, -1, nullptr, 0, 0, ix, nullptr, nullptr, nullptr) == WH_EINVAL);
  EXPECT(T.check() == 0);
}

}  // namespace

int main() {
  for (int64_t count : {(int64_t)1, (int64_t)16, (int64_t)17, (int64_t)333, (int64_t)4099, (int64_t)65537, (int64_t)1048577})
    exercise(count, 40 + (uint64_t)count);
  int64_t lw = 0, nw = 0;
  int32_t lv = 0;
  EXPECT(wh_replay_prio_query(0, &lw, &nw, &lv) == WH_EINVAL);
  EXPECT(wh_replay_prio_query(WH_PRIO_MAX_COUNT + 1, &lw, &nw, &lv) == WH_EINVAL);
  EXPECT(wh_replay_prio_query(WH_PRIO_MAX_COUNT, &lw, &nw, &lv) == WH_OK && lv == 8 && lw == WH_PRIO_MAX_COUNT);
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("ASAN PRIO OK\n");
  return 0;
}
