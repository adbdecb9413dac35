// step_params.h -- the argument of every step kernel (StepParams) and the episode-metrics fold
// (flush_episodes) (device code; included by warehouse_amd.hip after step_env.h and before
// step_wide.h, which uses both).
struct StepParams {
  uint32_t* state;
  int64_t B;
  int32_t na, T, W;
  const uint32_t* tables;
  const int32_t* actions;
  const int32_t* order;
  int32_t ol;               // order row length (1 .. 4 * NA; resolve_step turns 0 into NA)
  float* rewards;
  uint8_t* dones;
  float* returns;
  const int32_t* regen;
  int32_t* n_inactive;
  int32_t* actions_out;
  float p;
  uint32_t k0, k1;
  int64_t env_offset;
  int32_t steps, phase, autoreset, variable_n;
  int32_t ablate;  // timing-only phase skips (env WH_ABLATE), never set in normal use
  wh_episode_stats stats;   // all-NULL = off
  const uint8_t* mask;      // [B] or NULL: envs to step (wh_vector_step)
  uint32_t* state_out;      // NULL: in place; else the state is read from `state`, written here
                            // (wh_sampler_step_to: double-buffered, no mask)
};

// Folds the episodes this wave finished into the per-n bins of wh_episode_stats (the
// on_episode_end metrics of scripts/train.py:18-23): one set of global atomics per distinct n in
// the wave.  Sums, minima and maxima are built from ballots over bit slices, so only active lanes
// contribute and the integer results do not depend on lane or wave order.
__device__ __forceinline__ void flush_episodes(bool fin, uint32_t n, uint32_t ret, const wh_episode_stats& st) {
  uint64_t pend = __ballot(fin);
  while (pend) {
    const int leader = __ffsll((unsigned long long)pend) - 1;
    const uint32_t nb = (uint32_t)__shfl((int)n, leader);
    const bool g = fin && n == nb;
    const uint64_t gm = __ballot(g);
    pend &= ~gm;
    uint64_t sum = 0;
    uint32_t mn = 0, mx = 0;
    bool cmin = g, cmax = g;
    for (int b = 31; b >= 0; --b) {
      const bool bit = (ret >> b) & 1u;
      sum += (uint64_t)__popcll(__ballot(g && bit)) << b;
      if (__ballot(cmax && bit)) { mx |= 1u << b; cmax = cmax && bit; }
      if (__ballot(cmin && !bit)) cmin = cmin && !bit;
      else mn |= 1u << b;
    }
    if ((int)__lane_id() == leader) {
      if (st.return_sum) atomicAdd(&st.return_sum[nb], (unsigned long long)sum);
      if (st.episodes) atomicAdd(&st.episodes[nb], (unsigned long long)__popcll(gm));
      if (st.return_min) atomicMin(&st.return_min[nb], mn);
      if (st.return_max) atomicMax(&st.return_max[nb], mx);
    }
  }
}
