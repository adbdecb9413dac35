// csrc/mlp_grid.h (how wh_mlp_forward_multi shares a launch's workgroups out among its jobs) under
// AddressSanitizer + UndefinedBehaviorSanitizer, stand-alone: every combination of 1..8 jobs' task
// counts drawn from {0, 1, 2, 3, C-1, C, C+1, 1000} would be 8^8 cases per cap, so the full product
// runs up to 4 jobs and a fixed-seed sample beyond; plus row counts up to 2^40.  Checked per case:
// first ascending from 0, 1 <= b_j <= T_j for a job with tasks (0 without), sum b_j <= C, b_j = T_j
// whenever sum T <= C, one job = min(T, C), the greedy rule's balance, and -- by walking tasks
// bid, bid + b_j, ... as the kernels do -- that every task of every job is visited exactly once.
// The f32 rule: b_j = ceil(ceil(rows / 32) / 4), no cap, a grid past INT32_MAX refused.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mlp_grid.h"

static int fails = 0;
#define CHECK(c, ...)                        \
  do {                                       \
    if (!(c)) {                              \
      if (++fails <= 20) {                   \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                 \
        printf("\n");                        \
      }                                      \
    }                                        \
  } while (0)

static void check_persistent(int n, const int64_t* T, int64_t C) {
  // exactly n + 1 entries on the heap: a write past first[n] is ASan's to report
  std::vector<int32_t> first(n + 1, -7);
  int64_t live = 0, sum = 0;
  for (int j = 0; j < n; ++j) {
    live += T[j] > 0;
    sum += T[j];
  }
  const bool ok = mlp_grid::persistent(n, T, C, first.data());
  if (live > C) {
    CHECK(!ok && first[0] == -7, "more live jobs than blocks must be refused");
    return;
  }
  CHECK(ok, "n=%d C=%lld refused", n, (long long)C);
  if (!ok) return;
  CHECK(first[0] == 0, "first[0]");
  int64_t total = 0;
  for (int j = 0; j < n; ++j) {
    const int64_t b = (int64_t)first[j + 1] - first[j];
    CHECK(b >= 0, "first not ascending at %d", j);
    if (T[j] == 0) CHECK(b == 0, "a job without tasks got %lld blocks", (long long)b);
    else CHECK(b >= 1 && b <= T[j], "job %d: b=%lld T=%lld", j, (long long)b, (long long)T[j]);
    if (sum <= C) CHECK(b == T[j], "sum T <= C: job %d b=%lld T=%lld", j, (long long)b, (long long)T[j]);
    total += b;
  }
  CHECK(total <= C && total == first[n], "sum b = %lld > C = %lld", (long long)total, (long long)C);
  if (sum > C) CHECK(total == C, "over the cap every block is given: %lld of %lld", (long long)total, (long long)C);
  if (n == 1) CHECK(total == (T[0] < C ? T[0] : C), "one job is the single launch's grid");
  // greedy balance: no job could hand a block to a more loaded one and lower the maximum of
  // tasks per block -- for a != c with b_a >= 2 and b_c < T_c: T_c / b_c <= T_a / (b_a - 1)
  for (int a = 0; a < n; ++a)
    for (int c = 0; c < n; ++c) {
      const int64_t ba = (int64_t)first[a + 1] - first[a], bc = (int64_t)first[c + 1] - first[c];
      if (a == c || ba < 2 || bc == 0 || bc >= T[c]) continue;
      CHECK((__int128)T[c] * (ba - 1) <= (__int128)T[a] * bc, "unbalanced: T=%lld b=%lld against T=%lld b=%lld",
            (long long)T[c], (long long)bc, (long long)T[a], (long long)ba);
    }
  // the strided walk of the kernels: block `blk` finds its job by the scan over first, then takes tasks
  // bid, bid + nblk, ... (my_tasks = (T - bid + nblk - 1) / nblk of them)
  for (int j = 0; j < n; ++j) {
    if (T[j] > 4096) continue;                         // (huge jobs: the counts below cover them)
    std::vector<uint8_t> seen((size_t)T[j], 0);
    for (int32_t blk = first[j]; blk < first[j + 1]; ++blk) {
      int jj = 0;
      for (int i = 1; i < n; ++i)
        if (blk >= first[i]) jj = i;
      // (trailing jobs without blocks share first[] values with their neighbours: the scan must
      // still land on the job that owns the block)
      CHECK((int64_t)first[jj + 1] - first[jj] > 0 && blk >= first[jj] && blk < first[jj + 1], "scan: block %d -> job %d", blk, jj);
      const int64_t bid = blk - first[jj], nblk = first[jj + 1] - first[jj];
      const int64_t mine = (T[jj] - bid + nblk - 1) / nblk;
      for (int64_t it = 0; it < mine; ++it) {
        const int64_t task = bid + it * nblk;
        CHECK(task < T[jj], "task %lld past T=%lld", (long long)task, (long long)T[jj]);
        if (task < T[jj] && jj == j) ++seen[(size_t)task];
      }
    }
    for (int64_t t = 0; t < T[j]; ++t) CHECK(seen[(size_t)t] == 1, "job %d task %lld visited %d times", j, (long long)t, seen[(size_t)t]);
  }
  for (int j = 0; j < n; ++j) {                        // the counts alone, any size
    const int64_t nblk = (int64_t)first[j + 1] - first[j];
    int64_t visited = 0;
    for (int64_t bid = 0; bid < nblk; ++bid) visited += (T[j] - bid + nblk - 1) / nblk;
    CHECK(visited == T[j], "job %d: %lld of %lld tasks walked", j, (long long)visited, (long long)T[j]);
  }
}

static void check_f32(int n, const int64_t* rows) {
  std::vector<int32_t> first(n + 1, -7);
  int64_t total = 0;
  for (int j = 0; j < n; ++j) total += ((rows[j] + 31) / 32 + 3) / 4;
  const bool ok = mlp_grid::per_tile(n, rows, first.data());
  if (total > INT32_MAX) {
    CHECK(!ok && first[0] == -7, "a grid past INT32_MAX blocks must be refused");
    return;
  }
  CHECK(ok && first[0] == 0, "f32 refused");
  if (!ok) return;
  for (int j = 0; j < n; ++j) {
    const int64_t b = (int64_t)first[j + 1] - first[j];
    CHECK(b == ((rows[j] + 31) / 32 + 3) / 4, "f32 job %d: b=%lld rows=%lld", j, (long long)b, (long long)rows[j]);
    // block bid's four waves take tiles 4 bid .. 4 bid + 3: the last block holds the last tile
    if (rows[j] > 0) CHECK((b - 1) * 128 < rows[j] && b * 128 >= rows[j], "f32 job %d covers its rows", j);
  }
}

int main() {
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&]() {
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return rng;
  };
  long cases = 0;
  for (const int64_t C : {8, 9, 64, 256}) {
    const int64_t draw[8] = {0, 1, 2, 3, C - 1, C, C + 1, 1000};
    int64_t T[mlp_grid::MAX_JOBS];
    for (int n = 1; n <= 4; ++n) {                       // the full product
      long combos = 1;
      for (int i = 0; i < n; ++i) combos *= 8;
      for (long c = 0; c < combos; ++c) {
        long v = c;
        for (int j = 0; j < n; ++j, v /= 8) T[j] = draw[v % 8];
        check_persistent(n, T, C);
        ++cases;
      }
    }
    for (int n = 5; n <= mlp_grid::MAX_JOBS; ++n)        // a fixed-seed sample
      for (int c = 0; c < 3000; ++c) {
        for (int j = 0; j < n; ++j) T[j] = draw[next() % 8];
        check_persistent(n, T, C);
        ++cases;
      }
    // the learner's cases: five equal jobs of 2 tasks (M = 64 Medium-8), three of 121 over the cap
    const int64_t five[5] = {2, 2, 2, 2, 2}, three[3] = {121, 121, 121};
    check_persistent(5, five, C);
    check_persistent(3, three, C);
    // row counts up to 2^40 through ceil_div, as the entry point does (256- and 128-row tasks)
    for (const int64_t per : {256, 128})
      for (int n = 1; n <= mlp_grid::MAX_JOBS; ++n) {
        int64_t rows[mlp_grid::MAX_JOBS];
        for (int j = 0; j < n; ++j) {
          rows[j] = (j % 3 == 0) ? ((int64_t)1 << 40) - j : (j % 3 == 1) ? (int64_t)(next() % 100000) : ((int64_t)1 << 31) + j;
          T[j] = mlp_grid::ceil_div(rows[j], per);
          CHECK(T[j] == (rows[j] + per - 1) / per, "ceil_div");
        }
        check_persistent(n, T, C);
        check_f32(n, rows);
        ++cases;
      }
  }
  CHECK(mlp_grid::ceil_div(0, 256) == 0 && mlp_grid::ceil_div(1, 256) == 1 && mlp_grid::ceil_div(256, 256) == 1 &&
        mlp_grid::ceil_div(257, 256) == 2 && mlp_grid::ceil_div(INT64_MAX, 32) == INT64_MAX / 32 + 1, "ceil_div edges");
  {                                                       // refusals write nothing
    int32_t first[mlp_grid::MAX_JOBS + 1] = {-7, -7, -7, -7, -7, -7, -7, -7, -7};
    const int64_t neg[2] = {3, -1}, nine[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
    CHECK(!mlp_grid::persistent(2, neg, 8, first) && !mlp_grid::per_tile(2, neg, first), "negative counts");
    CHECK(!mlp_grid::persistent(9, nine, 256, first) && !mlp_grid::per_tile(9, nine, first), "nine jobs");
    CHECK(!mlp_grid::persistent(-1, nine, 256, first) && !mlp_grid::per_tile(-1, nine, first), "n < 0");
    CHECK(!mlp_grid::persistent(8, nine, 7, first), "eight live jobs, seven blocks");
    for (int i = 0; i < 9; ++i) CHECK(first[i] == -7, "a refusal wrote first[%d]", i);
    CHECK(mlp_grid::persistent(0, nine, 256, first) && first[0] == 0, "no job: an empty grid");
  }
  {                                                       // the f32 rule on small shapes
    const int64_t rows[6] = {0, 1, 31, 128, 129, 300};
    check_f32(6, rows);
    const int64_t big[8] = {(int64_t)1 << 40, (int64_t)1 << 40, 5, 0, 0, 0, 0, 0};   // 2^34 blocks: refused
    check_f32(8, big);
    const int64_t edge[2] = {(int64_t)INT32_MAX * 128, 0};                             // exactly INT32_MAX blocks
    check_f32(2, edge);
    const int64_t over[2] = {(int64_t)INT32_MAX * 128, 1};
    check_f32(2, over);
  }
  if (fails) {
    printf("%d failures\n", fails);
    return 1;
  }
  printf("ASAN MLP GRID OK (%ld cases)\n", cases);
  return 0;
}
