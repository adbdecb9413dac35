// step_record.h -- the recorded step (device code; included by warehouse_amd.hip after step_loops.h,
// whose step it runs, and replay.h, whose record layout and SmallDiv it uses): RecordParams,
// tile_from_raw / tile_from_regs, write_records, k_step_record.
//
// wh_replay_record: `steps` times [policy ->] put(stage 0) -> step without auto-reset -> put(stage 1)
// -> reset of the done envs, as ONE launch.  The put launches re-read from HBM a state the step
// launch held in registers a moment earlier; here the lane that steps an env writes both of the
// slot's records from its registers and its pickup plane, through the LDS transpose k_replay_put does.

// The argument of k_step_record: the step's own StepParams (its kernarg layout stays what every step
// kernel reads) and the ring.
struct RecordParams {
  StepParams s;
  uint32_t* r_states;   // the ring (wh_replay_ring)
  uint8_t* r_actions;
  float* r_rewards;
  uint8_t* r_dones;
  int64_t slot, capacity;   // step k records into slot (slot + k) % capacity
  int32_t words;            // packed words per env: 2 + na + 2 * PW
};

// An env's packed words in the order store_env writes its planes (include/warehouse_amd.h, PACKED
// STATE): header, episode counter, the na agent words, PW target words, PW expiry words.  A lane's
// row of the tile is `stride` words, odd, so the lanes of a wave write every word to 64 different
// banks (k_replay_put's padding).
template <class C>
__device__ __forceinline__ void tile_from_raw(uint32_t* row, const RawEnv<C>& r, int na) {
  row[0] = r.hdr;
  row[1] = r.epi;
#pragma unroll
  for (int i = 0; i < C::NAM; ++i)
    if (i < na) row[2 + i] = r.ag[i];
  uint32_t* pt = row + 2 + na;
#pragma unroll
  for (int w = 0; w < C::PW; ++w) {
    pt[w] = r.pt[w];
    pt[C::PW + w] = r.pm[w];
  }
}

template <class C>
__device__ __forceinline__ void tile_from_regs(uint32_t* row, const Regs<C>& s, const Lds<C>& L, int na, int tid) {
  row[0] = s.hdr;
  row[1] = s.epi;
#pragma unroll
  for (int i = 0; i < C::NAM; ++i)
    if (i < na) row[2 + i] = s.ag[i];
  uint32_t* pt = row + 2 + na;
#pragma unroll
  for (int w = 0; w < C::PW; ++w) {
    // four 16-bit cells -> target bytes and expiry bytes (store_env)
    const uint32_t lo = (uint32_t)L.pkp[4 * w][tid] | ((uint32_t)L.pkp[4 * w + 1][tid] << 16);
    const uint32_t hi = (uint32_t)L.pkp[4 * w + 2][tid] | ((uint32_t)L.pkp[4 * w + 3][tid] << 16);
    pt[w] = __builtin_amdgcn_perm(hi, lo, 0x06040200u);
    pt[C::PW + w] = __builtin_amdgcn_perm(hi, lo, 0x07050301u);
  }
}

// The workgroup's nenv records -- contiguous in the ring -- from the tile, as consecutive words
// (every lane of the workgroup, whether it holds an env or not)
template <int STRIDE>
__device__ __forceinline__ void write_records(const uint32_t* tile, uint32_t* __restrict__ out, uint32_t nenv,
                                              uint32_t words, int tid) {
  const uint32_t total = nenv * words;
  const SmallDiv by_words(words);
  for (uint32_t j = tid; j < total; j += BT) {
    const uint32_t el = by_words(j), w = j - el * words;
    out[j] = tile[el * STRIDE + w];
  }
}

// One lane per env, a.steps recorded steps.  Every lane of the workgroup reaches every barrier: a
// lane past B re-reads env e0 (k_sampler's generic branch) and skips the step body, so a wave-wide
// operation inside the body sees only lanes with an env, as in k_step.  Per step: side 0 into the
// tile | barrier | side-0 records out, moves, actions, step, rewards / dones, episode metrics |
// barrier | side 1 into the tile | barrier | side-1 records out, reset of a done env | barrier.
template <class C, int POLICY>
__global__ __launch_bounds__(BT) void k_step_record(RecordParams p) {
  constexpr int WMAX = 2 + C::NAM + 2 * C::PW, STRIDE = WMAX | 1;
  static_assert(sizeof(Lds<C>) + sizeof(uint32_t) * BT * STRIDE <= 160 * 1024,
                "k_step_record exceeds the LDS of a workgroup");
  __shared__ Lds<C> L;
  __shared__ uint32_t tile[BT * STRIDE];
  const StepParams& a = p.s;
  const int tid = threadIdx.x;
  const int64_t e0 = (int64_t)blockIdx.x * BT;
  const int64_t e = e0 + tid;
  const bool loaded = e < a.B;
  const int na = a.na;
  const uint4 tv0 = issue_table_chunk<C>(a.tables, 0), tv1 = issue_table_chunk<C>(a.tables, 1);
  __builtin_amdgcn_sched_barrier(0);   // table loads ahead of the state loads, as in k_step
  RawEnv<C> raw;
  load_env_issue<C>(raw, a.state, a.B, e0, loaded ? tid : 0, na);
  commit_table_chunk<C>(L.tbl, 0, tv0);
  commit_table_chunk<C>(L.tbl, 1, tv1);
#pragma unroll
  for (int y = 0; y < C::D; ++y) L.occ[y][tid] = 0u;   // occupancy grid starts empty (step_env)
  uint32_t* row = tile + tid * STRIDE;
  if (loaded) tile_from_raw<C>(row, raw, na);   // side 0 of the first step: the words just loaded
  __syncthreads();
  const uint32_t nenv = (uint32_t)((a.B - e0) < BT ? (a.B - e0) : BT);
  const uint32_t words = (uint32_t)p.words;
  const Keys k{a.k0, a.k1};
  const uint32_t gid = (uint32_t)(a.env_offset + e);
  Regs<C> s;
  const bool stats = loaded && a.stats.episode_return != nullptr;
  uint32_t epr = 0;
  if (loaded) {
    load_env_finish<C>(s, L, raw, (uint32_t)a.W, tid);
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): drain the state loads before the step (k_step)
    if (stats) epr = a.stats.episode_return[e];
  }
  int64_t slot = p.slot;
  for (int stp = 0; stp < a.steps; ++stp) {
    if (stp > 0) {
      if (loaded) tile_from_regs<C>(row, s, L, na, tid);
      __syncthreads();
    }
    const int64_t ent = slot * a.B;   // the slot's first entry
    write_records<STRIDE>(tile, p.r_states + (2 * ent + e0) * words, nenv, words, tid);
    bool done = false;
    if (loaded) {
      uint32_t d[C::NAM];
      uint8_t* ract = p.r_actions + (ent + e) * na;
      if (POLICY == POL_EXTERNAL) {
#pragma unroll
        for (int i = 0; i < C::NAM; ++i) {
          const uint32_t act = valid_action(i < na ? (uint32_t)a.actions[e * na + i] : 4u);
          if (i < na) ract[i] = (uint8_t)act;
          d[i] = L.mv(act);
        }
      } else {
        // the actions wh_policy reports: the drawn action itself (EFF = false), 4 for slots >= n
        // (Greedy: the walk made here and handed over, which is policy_steps' own code in another
        // instantiation.  As a second caller of k_step's <C, POL_GREEDY> one, this kernel changed the
        // register allocation of every generic greedy k_step instance: tools/isa_compare.py.)
        if constexpr (POLICY == POL_GREEDY) {
          uint32_t wrp[C::R], wtg[C::R];
          policy_walk<C>(s, L, wrp, wtg);
          policy_steps<C, POLICY, false, true>(s, L, k, gid, a.p, d, &wrp, &wtg);
        } else {
          policy_steps<C, POLICY>(s, L, k, gid, a.p, d);
        }
        const uint32_t n = (s.hdr >> 16) & 0xFFu;
#pragma unroll
        for (int i = 0; i < C::NAM; ++i)
          if (i < na) ract[i] = (uint8_t)(i < (int)n ? action_of(d[i]) : 4u);
      }
      float rew[C::NAM];
      done = step_env<C, false, true, true>(s, L, d, OrderIn{nullptr, 0, nullptr}, a.actions, nullptr, k, gid, e, na,
                                            PH_ALL, (uint32_t)a.T, (uint32_t)a.W, rew, nullptr, tid, 0);
      store_rewards<C>(L, rew, p.r_rewards + ent * na, a.B, e, na, tid, false);
      p.r_dones[ent + e] = done ? 1 : 0;
      if (a.rewards) store_rewards<C>(L, rew, a.rewards + (int64_t)stp * a.B * na, a.B, e, na, tid, false);
      if (a.dones) a.dones[(int64_t)stp * a.B + e] = done ? 1 : 0;
      if (stats) {
        float r = 0.0f;
#pragma unroll
        for (int i = 0; i < C::NAM; ++i) r += rew[i];   // whole numbers: exact
        epr += (uint32_t)r;
        if (__any(done)) flush_episodes(done, (s.hdr >> 16) & 0xFFu, epr, a.stats);
        if (done) epr = 0;
      }
    }
    __syncthreads();   // the side-0 records have left the tile
    if (loaded) tile_from_regs<C>(row, s, L, na, tid);   // the stepped state, before any reset
    __syncthreads();
    write_records<STRIDE>(tile, p.r_states + (2 * ent + a.B + e0) * words, nenv, words, tid);
    if (loaded && done) {
      reset_philox<C>(s, L, k, gid, na, a.variable_n, (uint32_t)a.W, tid);
#pragma unroll
      for (int y = 0; y < C::D; ++y) L.occ[y][tid] = 0u;
    }
    if (loaded) WH_CHECK_ENV(s, L, e, tid);
    slot = slot + 1 == p.capacity ? 0 : slot + 1;
    __syncthreads();   // the side-1 records have left the tile
  }
  if (loaded) {
    if (stats) a.stats.episode_return[e] = epr;
    store_env<C>(s, L, a.state, a.B, e0, na, tid);
  }
}
