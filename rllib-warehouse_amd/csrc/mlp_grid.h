// mlp_grid.h -- how one wh_mlp_forward_multi launch shares its workgroups out among its jobs.  Plain
// C++17 with no HIP in it: policy_mlp.hip includes it for the launch, tests/asan/mlp_grid_asan.cpp to
// check it on a CPU.  Needs <stdint.h>.
//
// A launch of n jobs is one grid whose blocks first[j] .. first[j + 1] - 1 belong to job j (first
// ascending, first[0] = 0, first[n] = the grid).  Results do not depend on the partition -- rows are
// independent and the sampler's philox is keyed by the absolute row -- so the rules only balance load.
#pragma once
#include <stdint.h>

namespace mlp_grid {

constexpr int MAX_JOBS = 8;   // == WH_MLP_MAX_JOBS (policy_mlp.hip asserts it)

// ceil(rows / per) for rows >= 0, without the overflow of rows + per - 1
inline int64_t ceil_div(int64_t rows, int64_t per) { return rows <= 0 ? 0 : (rows - 1) / per + 1; }

// The persistent kernels (bf16): job j has tasks[j] row tasks, and its b_j blocks walk them with the
// job-local stride b_j (block bid takes bid, bid + b_j, ...), each task exactly once.  With `cap`
// blocks to give (one per CU):
//   sum(tasks) <= cap: b_j = tasks[j], every task its own block, as a single launch would;
//   else every job with tasks gets one block and the other cap - live go one at a time to the job with
//   the most tasks per block (ties: the lowest j), no job beyond b_j = tasks[j].
// So 1 <= b_j <= tasks[j] for a job with tasks (0 for one without), sum(b_j) <= cap.  For one job this
// is min(tasks, cap), the single launch's grid.  False (nothing written) when n is out of range, a
// task count is negative, or cap cannot give every job with tasks a block.
inline bool persistent(int n, const int64_t* tasks, int64_t cap, int32_t* first) {
  if (n < 0 || n > MAX_JOBS || cap > INT32_MAX) return false;
  int64_t b[MAX_JOBS] = {};
  int64_t total = 0, live = 0;
  bool fits = true;                       // sum(tasks) <= cap, without summing past it
  for (int j = 0; j < n; ++j) {
    if (tasks[j] < 0) return false;
    live += tasks[j] > 0;
    if (fits && tasks[j] <= cap - total) total += tasks[j];
    else fits = false;
  }
  if (live > cap) return false;
  if (fits) {
    for (int j = 0; j < n; ++j) b[j] = tasks[j];
  } else {
    for (int j = 0; j < n; ++j) b[j] = tasks[j] > 0;
    for (int64_t left = cap - live; left > 0; --left) {
      int best = -1;                      // tasks[best] / b[best] the largest, by cross-multiplication
      for (int j = 0; j < n; ++j) {       // (tasks < 2^63 / cap: rows are int64 and a task has >= 32)
        if (b[j] == 0 || b[j] >= tasks[j]) continue;
        if (best < 0 || (__int128)tasks[j] * b[best] > (__int128)tasks[best] * b[j]) best = j;
      }
      if (best < 0) break;                // (cannot happen here: sum(b) < cap < sum(tasks))
      ++b[best];
    }
  }
  first[0] = 0;
  for (int j = 0; j < n; ++j) first[j + 1] = first[j] + (int32_t)b[j];
  return true;
}

// The f32 kernel: not persistent, one wave per 32-row tile and four waves per block, so
// b_j = ceil(ceil(rows_j / 32) / 4) as the single launch has it, with no cap.  False (nothing
// written) when n is out of range, a row count is negative or the grid would pass INT32_MAX blocks.
inline bool per_tile(int n, const int64_t* rows, int32_t* first) {
  if (n < 0 || n > MAX_JOBS) return false;
  int64_t total = 0;
  for (int j = 0; j < n; ++j) {
    if (rows[j] < 0) return false;
    total += ceil_div(ceil_div(rows[j], 32), 4);   // (8 x 2^63 / 128 cannot overflow)
  }
  if (total > INT32_MAX) return false;
  first[0] = 0;
  for (int j = 0; j < n; ++j) first[j + 1] = first[j] + (int32_t)ceil_div(ceil_div(rows[j], 32), 4);
  return true;
}

}  // namespace mlp_grid
