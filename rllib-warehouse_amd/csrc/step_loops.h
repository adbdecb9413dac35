// step_loops.h -- the step loops and the kernels around them (device code; included by
// warehouse_amd.hip after reset.h, policy.h, step_env.h and step_params.h): run_steps, the fused
// rollout's FastRun and run_steps_fast, k_step, k_reset, and the WH_TIMING stamps.

// The ablation word of a launch (tools/ablate.py: timing-only phase skips), the constant 0 in every
// build without -DWH_ABLATION, where the tests of it fold away.  (A macro like WH_CHECK_ENV: as an
// inline function it commuted operands in the ablation build's step kernels.)
#ifdef WH_ABLATION
#define WH_ABLATE_WORD(a) ((a).ablate)
#else
#define WH_ABLATE_WORD(a) 0
#endif

// MOVES[action] as the packed step (core.py:38)
template <class C>
__device__ __forceinline__ uint32_t move_of(const Lds<C>& L, uint32_t action) {
  return L.mv(valid_action(action));
}

// the ablation's stand-in for a policy (ablate & 1): moves that cost nothing to compute
template <class C>
__device__ __forceinline__ void ablation_moves(const Lds<C>& L, int stp, uint32_t (&d)[C::NAM]) {
#pragma unroll
  for (int i = 0; i < C::NAM; ++i) d[i] = L.mv((uint32_t)((i + stp) % 9));
}

// The step loop of k_step.  PHASE >= 0 fixes the phase at compile time (the fused rollout and the
// sampler path run PH_ALL), so the phase tests fold away and each step is a few large basic blocks
// the scheduler can interleave; -1 reads it from the launch (the drop-in's split step).  Phase
// ablation (tools/ablate.py) exists only in builds with -DWH_ABLATION.
template <class C, int POLICY, bool ORDERED, int PHASE>
__device__ __forceinline__ void run_steps(const StepParams& a, Regs<C>& s, Lds<C>& L, const Keys& k,
                                          uint32_t gid, int64_t e, int tid, uint16_t* okeys = nullptr) {
  const int phase = PHASE >= 0 ? PHASE : a.phase;
  const OrderIn oi{a.order, a.ol, okeys};
  const int ablate = WH_ABLATE_WORD(a);
  float ret = 0.0f;
  const bool stats = a.stats.episode_return != nullptr;
  uint32_t epr = stats ? a.stats.episode_return[e] : 0u;
  for (int stp = 0; stp < a.steps; ++stp) {
    uint32_t d[C::NAM];
    if (POLICY == POL_EXTERNAL) {
      const bool have = phase != PH_REGEN && !ORDERED;   // REGEN reads no actions
#pragma unroll
      for (int i = 0; i < C::NAM; ++i) {
        d[i] = move_of<C>(L, (have && i < a.na) ? (uint32_t)a.actions[e * a.na + i] : 4u);
      }
    } else if (ablate & 1) {
      ablation_moves<C>(L, stp, d);
    } else {
      policy_steps<C, POLICY, POLICY == POL_GREEDY && !kAblationBuild>(s, L, k, gid, a.p, d);
    }
    float rew[C::NAM];
    const bool done = step_env<C, ORDERED, true, POLICY != POL_GREEDY || kAblationBuild>(s, L, d, oi, a.actions, a.regen, k, gid, e, a.na, phase,
                                  (uint32_t)a.T, (uint32_t)a.W, rew, a.n_inactive, tid, ablate);
    if (phase != PH_REGEN) {
      if (a.rewards && !(ablate & 64))
        store_rewards<C>(L, rew, a.rewards + (int64_t)stp * a.B * a.na, a.B, e, a.na, tid, a.mask != nullptr);
      if (a.dones && !(ablate & 64)) a.dones[(int64_t)stp * a.B + e] = done ? 1 : 0;
      if (a.returns) {
#pragma unroll
        for (int i = 0; i < C::NAM; ++i) ret += rew[i];
      }
      if (stats) {
        float r = 0.0f;
#pragma unroll
        for (int i = 0; i < C::NAM; ++i) r += rew[i];   // whole numbers: exact
        epr += (uint32_t)r;
        if (__any(done)) flush_episodes(done, (s.hdr >> 16) & 0xFFu, epr, a.stats);
        if (done) epr = 0;
      }
      if (done && a.autoreset && !(ablate & 128)) {
        reset_philox<C>(s, L, k, gid, a.na, a.variable_n, (uint32_t)a.W, tid);
#pragma unroll
        for (int y = 0; y < C::D; ++y) L.occ[y][tid] = 0u;
      }
    }
    if (phase != PH_PRE) WH_CHECK_ENV(s, L, e, tid);
  }
  if (a.returns) a.returns[e] += ret;
  if (stats) a.stats.episode_return[e] = epr;
}

// The fused rollout's common case as its own instance: wh_rollout with rewards + dones written,
// auto-reset on, no returns / episode stats / env mask, na == NAM with NAM even (16/8-byte reward
// rows).  No per-step tests of launch options, and the injected-draw path is compiled out, so a
// step executes few branch instructions -- each costs several issue slots at one wave per SIMD
// (tools/oprate5.hip: ~8 ns per s_cbranch/s_branch against ~2.6 ns per VALU op).  Its steps keep the
// grid between them (step_env's LAZY form).

// Lanes of a wave ending their episodes in the same step that are reset one at a time from their
// reset slots (~40 issue slots each); more than this take the all-lane reset_philox (~700 VALU).
constexpr int kSlotResetMax = 8;
// A fill costs about two single-lane resets and a launch of K desynchronised steps ends ~K/3 episodes
// per wave (Medium-8), so launches shorter than this reset single lanes from scratch (reset_lane).
constexpr int kSlotMinSteps = 8;

// The ended-episode reset dispatch ("which reset form does this wave take") is written out twice, in
// FastRun::step and in run_steps_fast: a change to one belongs in the other.  As one __forceinline__
// helper called from both, every fast k_step instance compiled to another register allocation (SGPR
// counts and spills changed in 27 kernels of the registry), so the twin stays.

// One step of the fused rollout's common case at a time (run_steps_fast loops over it; k_sampler
// interleaves it with writing observation rows).  Carries the lazy grid and the output rows.
// SLOTS = false: no reset slots -- a lone ending lane is reset by reset_lane, as launches shorter
// than kSlotMinSteps do.
template <class C, int POLICY, bool SLOTS = true>
struct FastRun {
  float* rrow;
  uint8_t* drow;
  int64_t rstride;
  LazyGrid lg;
  uint32_t act[POLICY == POL_EXTERNAL ? C::NAM : 1];   // external actions of the (single) step
  __device__ __forceinline__ FastRun(const StepParams& a, int64_t e)
      : rrow(a.rewards + e * C::NAM), drow(a.dones + e), rstride(a.B * C::NAM), lg{true, 0u, false} {}   // the grid starts empty (k_step)
  // POL_EXTERNAL: the step's actions, loaded with the state in the prologue (their HBM latency then
  // overlaps the table loads instead of sitting on the first step)
  __device__ __forceinline__ void load_actions(const StepParams& a, int64_t e) {
    if constexpr (POLICY == POL_EXTERNAL) {
      if constexpr (C::NAM % 4 == 0) {
        const uint4* src = reinterpret_cast<const uint4*>(a.actions + e * C::NAM);
#pragma unroll
        for (int q = 0; q < C::NAM / 4; ++q) {
          const uint4 v = src[q];
          act[4 * q] = v.x; act[4 * q + 1] = v.y; act[4 * q + 2] = v.z; act[4 * q + 3] = v.w;
        }
      } else {
        const uint2* src = reinterpret_cast<const uint2*>(a.actions + e * C::NAM);
#pragma unroll
        for (int q = 0; q < C::NAM / 2; ++q) {
          const uint2 v = src[q];
          act[2 * q] = v.x; act[2 * q + 1] = v.y;
        }
      }
    }
  }

  __device__ __forceinline__ void step(const StepParams& a, Regs<C>& s, Lds<C>& L, Slots<C>* RS, const Keys& k,
                                       uint32_t gid, int64_t e, int tid, int stp) {
    const int ablate = WH_ABLATE_WORD(a);
    uint32_t d[C::NAM];
    if constexpr (POLICY == POL_EXTERNAL) {
#pragma unroll
      for (int i = 0; i < C::NAM; ++i) d[i] = move_of<C>(L, act[i]);
    } else if (ablate & 1) {
      ablation_moves<C>(L, stp, d);
    } else {
      policy_steps<C, POLICY, POLICY == POL_GREEDY && !kAblationBuild>(s, L, k, gid, a.p, d);
    }
    float rew[C::NAM];
    const bool done = step_env_fused<C, POLICY != POL_GREEDY || kAblationBuild>(s, L, d, k, gid, e, (uint32_t)a.T, (uint32_t)a.W, rew, tid,
                                                                                 ablate, &lg, nullptr, nullptr);
    if (!(ablate & 64)) {
      store_row<C>(rrow, rew);
      *drow = done ? 1 : 0;
    }
    rrow += rstride;
    drow += a.B;
    if (!(ablate & 128) && WH_RARE(__any(done))) {   // wave-uniform test first: one branch on the common path
      const uint64_t dm = __ballot(done);
      // a few envs of a full wave end (desynchronised episodes): wave-wide resets of them, one env
      // at a time (every lane takes part, so not in a tail wave whose lanes past B have exited)
      const bool full = __ballot(true) == ~0ull;
      // every form below clears grid columns of the lanes it resets; the flag is the wave's (LazyGrid),
      // so it is set here, outside the per-lane branches
      lg.rebuild = true;
      if (SLOTS && a.steps >= kSlotMinSteps && __popcll(dm) <= kSlotResetMax && full) {
        // their precomputed next-episode states, after (re)filling the wave's slots if one of
        // theirs is stale: one wave-wide fill (every lane's next episode) serves the resets of
        // the lanes that end later in this launch
        if constexpr (SLOTS) {
          if (__any(done && RS->rs_ep[tid] != s.epi + 1u))
            reset_philox<C, C::NAM, true>(s, L, k, gid, C::NAM, a.variable_n, (uint32_t)a.W, tid, RS);
          for (uint64_t m = dm; m; m &= m - 1ull) reset_from_slot<C, C::NAM>(s, L, *RS, (uint32_t)a.W, tid, __builtin_ctzll(m));
        }
      } else if (__popcll(dm) == 1 && full) {
        // short launches (the sampler's 1-step ones): a fill would serve few later resets
        reset_lane<C, C::NAM>(s, L, k, gid, a.variable_n, (uint32_t)a.W, tid, __builtin_ctzll(dm));
      } else if (dm == ~0ull) {
        // every lane of the wave (synchronised episodes): the grid and pickup plane cleared wave-wide
        reset_philox<C, C::NAM, false, true>(s, L, k, gid, C::NAM, a.variable_n, (uint32_t)a.W, tid);
      } else if (done) {
        reset_philox<C, C::NAM>(s, L, k, gid, C::NAM, a.variable_n, (uint32_t)a.W, tid);
#pragma unroll
        for (int y = 0; y < C::D; ++y) L.occ[y][tid] = 0u;
      }
    }
    WH_CHECK_ENV(s, L, e, tid);
  }
};

// k_step's fused rollout loop: FastRun's step, written out as one loop (the same body as a member
// call measured 2 % slower per step at Medium-8: profiles/r04_fastrun_ab.txt).
// EPS = false: the launch's exploration rate is 0 (resolve_step), so the greedy policy's random-move
// block and its per-step test of the rate are compiled out.
template <class C, int POLICY, bool SLOTS = true, bool EPS = true>
__device__ __forceinline__ void run_steps_fast(const StepParams& a, Regs<C>& s, Lds<C>& L, Slots<C>* RS,
                                               const Keys& k, uint32_t gid, int64_t e, int tid) {
  const int ablate = WH_ABLATE_WORD(a);
  // output rows of step stp: wave-uniform bases (scalar adds per step) + the lane's offset
  float* rrow = a.rewards + (e - tid) * C::NAM;
  uint8_t* drow = a.dones + (e - tid);
  const int64_t rstride = a.B * C::NAM;
  LazyGrid lg{true, 0u, false};   // the grid starts empty (k_step)
  EnvConst<C> ec;   // n changes only in a reset
  ec.set(s.hdr);
  // ROT: the greedy loop is rotated.  The request walk of step t + 1 (policy_walk: nine dependent LDS
  // lookups) is issued right after step t's regeneration, and its results cross the back-edge in
  // registers, so their latency is behind the loop branch instead of in front of the policy's distance
  // tests.  The first step's walk is made here, and a reset's -- which replaces the request mask and
  // sets `fresh` -- after it.
  constexpr bool ROT = POLICY == POL_GREEDY && !kAblationBuild;
  [[maybe_unused]] uint32_t wrp[C::R], wtg[C::R];
  if constexpr (ROT) policy_walk<C>(s, L, wrp, wtg);
  for (int stp = 0; stp < a.steps; ++stp) {
    uint32_t d[C::NAM];
    if constexpr (POLICY == POL_EXTERNAL) {   // (wh_vector_step's fast case: one step)
#pragma unroll
      for (int i = 0; i < C::NAM; ++i) d[i] = move_of<C>(L, (uint32_t)a.actions[e * C::NAM + i]);
    } else if (ablate & 1) {
      ablation_moves<C>(L, stp, d);
    } else if constexpr (ROT) {
      policy_steps<C, POLICY, true, true, EPS>(s, L, k, gid, a.p, d, &wrp, &wtg);
    } else {
      policy_steps<C, POLICY, POLICY == POL_GREEDY && !kAblationBuild, false, EPS>(s, L, k, gid, a.p, d);
    }
    // The regeneration almost always draws (some lane of the wave reopens a point on nearly every
    // step), so its first Philox block -- a chain of ten dependent rounds -- is computed here, where
    // it fills the policy block's issue gaps: -0.5 % per step at Medium-8 and Large-16 against the
    // move loop's block (profiles/r05_step3_ab.txt).  Pinned: LLVM would sink it to its use.
    uint4 rb = stream_block(k, gid, s.epi, (s.hdr + 1u) & 0xFFFFu, PUR_REGEN, 0u);
    asm volatile("" : "+v"(rb.x), "+v"(rb.y), "+v"(rb.z), "+v"(rb.w));
    float rew[C::NAM];
    const bool done = step_env_fused<C, POLICY != POL_GREEDY || kAblationBuild>(s, L, d, k, gid, e, (uint32_t)a.T, (uint32_t)a.W, rew, tid,
                                                                                 ablate, &lg, &rb, &ec);
    if constexpr (ROT) policy_walk<C, true>(s, L, wrp, wtg);   // the next step's (redone below after a reset)
    if (!(ablate & 64)) {
      store_row<C>(rrow + tid * C::NAM, rew);
      drow[tid] = done ? 1 : 0;
    }
    rrow += rstride;
    drow += a.B;
    if (!(ablate & 128) && WH_RARE(__any(done))) {   // wave-uniform test first: one branch on the common path
      const uint64_t dm = __ballot(done);
      // a few envs of a full wave end (desynchronised episodes): wave-wide resets of them, one env
      // at a time (every lane takes part, so not in a tail wave whose lanes past B have exited)
      const bool full = __ballot(true) == ~0ull;
      // every form below clears grid columns of the lanes it resets; the flag is the wave's (LazyGrid),
      // so it is set here, outside the per-lane branches
      lg.rebuild = true;
      if (SLOTS && a.steps >= kSlotMinSteps && __popcll(dm) <= kSlotResetMax && full) {
        // their precomputed next-episode states, after (re)filling the wave's slots if one of
        // theirs is stale: one wave-wide fill (every lane's next episode) serves the resets of
        // the lanes that end later in this launch
        if constexpr (SLOTS) {
          if (__any(done && RS->rs_ep[tid] != s.epi + 1u))
            reset_philox<C, C::NAM, true>(s, L, k, gid, C::NAM, a.variable_n, (uint32_t)a.W, tid, RS);
          for (uint64_t m = dm; m; m &= m - 1ull) reset_from_slot<C, C::NAM>(s, L, *RS, (uint32_t)a.W, tid, __builtin_ctzll(m));
        }
      } else if (__popcll(dm) == 1 && full) {
        // short launches (the sampler's 1-step ones): a fill would serve few later resets
        reset_lane<C, C::NAM>(s, L, k, gid, a.variable_n, (uint32_t)a.W, tid, __builtin_ctzll(dm));
      } else if (dm == ~0ull) {
        // every lane of the wave (synchronised episodes): the grid and pickup plane cleared wave-wide
        reset_philox<C, C::NAM, false, true>(s, L, k, gid, C::NAM, a.variable_n, (uint32_t)a.W, tid);
      } else if (done) {
        reset_philox<C, C::NAM>(s, L, k, gid, C::NAM, a.variable_n, (uint32_t)a.W, tid);
#pragma unroll
        for (int y = 0; y < C::D; ++y) L.occ[y][tid] = 0u;
      }
      if constexpr (ROT) policy_walk<C>(s, L, wrp, wtg);   // of the states the resets left
      ec.set(s.hdr);
    }
    WH_CHECK_ENV(s, L, e, tid);
  }
}


// -DWH_TIMING builds (tools/launch_timeline.py): per-wave s_memrealtime stamps (100 MHz) of the fused
// rollout's phases -- entry, tables in LDS, state loaded, step loop done, state stored -- read back
// with wh_debug_times.  Written by lane 0 of each wave with vector stores.
#ifdef WH_TIMING
constexpr int kTimeSlots = 6, kTimeWaves = 4096;
__device__ unsigned long long g_wh_times[kTimeWaves * kTimeSlots];
#define WH_T(i)                                                                                   \
  do {                                                                                            \
    const unsigned long long now_ = __builtin_amdgcn_s_memrealtime();                             \
    const int w_ = (int)blockIdx.x * (BT / 64) + (int)(threadIdx.x >> 6);                        \
    if ((threadIdx.x & 63) == 0 && w_ < kTimeWaves) g_wh_times[w_ * kTimeSlots + (i)] = now_;     \
  } while (0)
#else
#define WH_T(i) ((void)0)
#endif

template <class C, int POLICY, bool ORDERED, bool FAST, bool EPS = true>
__global__ __launch_bounds__(BT) void k_step(StepParams a) {
  static_assert(EPS || (FAST && POLICY == POL_GREEDY), "the eps = 0 form exists for the fused greedy rollout only");
  __shared__ Lds<C> L;
  __shared__ std::conditional_t<FAST, Slots<C>, NoSlots> RS;   // reset slots: fused rollout only
  __shared__ std::conditional_t<ORDERED, OKeys<C>, NoSlots> OK;   // dict-order move keys: ORDERED only
  const int tid = threadIdx.x;
  if (FAST) WH_T(0);
  const int64_t e = (int64_t)blockIdx.x * BT + tid;
  const bool live = e < a.B && (FAST || !a.mask || a.mask[e]);
  const int na = FAST ? C::NAM : a.na;   // the fast instance runs na == NAM only (resolve_step)
  const int64_t e0 = (int64_t)blockIdx.x * BT;
  // Prologue: the table loads (L2) first, then the state planes (HBM); the table is written to LDS
  // and the occupancy grid cleared while the state is still in flight, and the pickup plane is
  // built as the state words land (the waitcnt pass counts each use against the in-order vmcnt).
  const uint4 tv0 = issue_table_chunk<C>(a.tables, 0), tv1 = issue_table_chunk<C>(a.tables, 1);
  __builtin_amdgcn_sched_barrier(0);   // keep the table loads ahead of the state loads
  // every lane loads (a lane past B or masked out re-reads env e0, which exists): a load under an exec
  // branch would make the waitcnt pass drain the state loads before the table's LDS writes
  RawEnv<C> raw;
  load_env_issue<C>(raw, a.state, a.B, e0, live ? tid : 0, na);
  commit_table_chunk<C>(L.tbl, 0, tv0);
  commit_table_chunk<C>(L.tbl, 1, tv1);
#pragma unroll
  for (int y = 0; y < C::D; ++y) L.occ[y][tid] = 0u;   // occupancy grid starts empty (step_env)
  __syncthreads();
  if (FAST) WH_T(1);
  if (!live) return;
  const Keys k{a.k0, a.k1};
  const uint32_t gid = (uint32_t)(a.env_offset + e);
  Regs<C> s;
  load_env_finish<C>(s, L, raw, (uint32_t)a.W, tid);
#ifdef WH_CHECK
  if (a.phase != PH_REGEN) WH_CHECK_ENV(s, L, e, tid);   // (a REGEN launch continues a PRE one)
  atomicAdd(&g_wh_check[3], (unsigned long long)a.steps + 1ull);
#endif
  // Drain the state loads here.  Their first uses are inside the step loop, so otherwise the
  // waitcnt pass places vmcnt waits in the loop body, where on every later iteration they also
  // wait for the previous step's reward/done stores to retire (a full memory round trip per step).
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0), expcnt/lgkmcnt untouched (gfx9 encoding)
  if constexpr (FAST) RS.rs_ep[tid] = s.epi;            // reset slots start stale (!= epi + 1)
  if (FAST) WH_T(2);

  if (!FAST && a.phase == PH_POLICY) {
    uint32_t d[C::NAM];
    policy_steps<C, POLICY>(s, L, k, gid, a.p, d);
    const uint32_t n = (s.hdr >> 16) & 0xFFu;
#pragma unroll
    for (int i = 0; i < C::NAM; ++i)
      if (i < a.na) a.actions_out[e * a.na + i] = (i < (int)n) ? (int32_t)action_of(d[i]) : 4;
    return;
  }

  if constexpr (FAST)
    run_steps_fast<C, POLICY, true, EPS>(a, s, L, &RS, k, gid, e, tid);
  else if (!ORDERED && a.phase == PH_ALL)
    run_steps<C, POLICY, ORDERED, PH_ALL>(a, s, L, k, gid, e, tid);
  else if constexpr (ORDERED)
    run_steps<C, POLICY, ORDERED, -1>(a, s, L, k, gid, e, tid, &OK.k[0][0]);
  else
    run_steps<C, POLICY, ORDERED, -1>(a, s, L, k, gid, e, tid);
  if (FAST) WH_T(3);
  store_env<C>(s, L, a.state_out ? a.state_out : a.state, a.B, e0, na, tid);
#ifdef WH_TIMING
  if (FAST) {
    __builtin_amdgcn_s_waitcnt(0);   // the state stores have left the wave
    WH_T(4);
  }
#endif
}

struct ResetParams {
  uint32_t* state;
  int64_t B;
  int32_t na, W;
  const uint32_t* tables;
  const uint8_t* mask;
  const int32_t *spawn, *pickups, *targets, *n;
  int32_t injected, variable_n;
  uint32_t k0, k1;
  int64_t env_offset;
};

template <class C>
__global__ __launch_bounds__(BT) void k_reset(ResetParams a) {
  __shared__ Lds<C> L;
  load_tables<C>(L.tbl, a.tables);
  __syncthreads();
  const int tid = threadIdx.x;
  const int64_t e = (int64_t)blockIdx.x * BT + tid;
  if (e >= a.B) return;
  if (a.mask && !a.mask[e]) return;
  Regs<C> s;
  s.epi = a.state[a.B + e];
  if (a.injected)
    reset_injected<C>(s, L, e, a.na, a.spawn, a.pickups, a.targets, a.n, (uint32_t)a.W, tid);
  else
    reset_philox<C>(s, L, Keys{a.k0, a.k1}, (uint32_t)(a.env_offset + e), a.na, a.variable_n,
                    (uint32_t)a.W, tid);
  if (!a.injected) WH_CHECK_ENV(s, L, e, tid);   // injected draws may legitimately be partial
  store_env<C>(s, L, a.state, a.B, (int64_t)blockIdx.x * BT, a.na, tid);
}
