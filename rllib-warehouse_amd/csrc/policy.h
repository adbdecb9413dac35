// policy.h -- the device policies (device code; included by warehouse_amd.hip after device_vocab.h):
// the greedy solver's request walk (policy_walk) and the unit steps of the greedy and random policies
// (policy_steps).
// ----------------------------------------------------------------------------- policy
// The greedy policy's request walk: the (at most R) open requests in ascending pickup order
// (core.py:409-418) as packed keys rp[] / tg[] for v_sad_hi_u8.  Index P of the tables is a
// sentinel (far-away cell, null-cell tag) that fills missing slots; after a reset every slot is
// the sentinel, so every agent's "nearest request" is the null cell, which is where the
// reference's reset observation sends the greedy solver (availability 0, core.py:233-236).
// Reads only the request mask and the fresh bit, so the fused step loop can run it for step t + 1
// as soon as step t's regeneration is done (run_steps_fast's ROT).
// STEPPED: the state comes straight out of a step, which clears the fresh bit, so the mask is used as
// it is (the bitop3 selects are opaque to LLVM: it cannot fold them on the constant).
template <class C, bool STEPPED = false>
__device__ __forceinline__ void policy_walk(const Regs<C>& s, const Lds<C>& L, uint32_t (&rp)[C::R],
                                            uint32_t (&tg)[C::R]) {
  const uint32_t mf = 0u - ((s.hdr >> 24) & 1u);
  uint32_t mlo = STEPPED ? (uint32_t)s.am : bop3<~TA & TB>(mf, (uint32_t)s.am, 0u);
  uint32_t mhi = STEPPED ? (uint32_t)(s.am >> 32) : bop3<~TA & TB>(mf, (uint32_t)(s.am >> 32), 0u);
#pragma unroll
  for (int r = 0; r < C::R; ++r) {
    uint32_t flo, fhi;
    asm("v_ffbl_b32 %0, %1" : "=v"(flo) : "v"(mlo));   // 0xFFFFFFFF when empty
    asm("v_ffbl_b32 %0, %1" : "=v"(fhi) : "v"(mhi));
    const uint32_t j = __builtin_elementwise_min(
        __builtin_elementwise_min(flo, __builtin_elementwise_add_sat(fhi, 32u)), (uint32_t)C::P);
    const uint2 v = L.rtag(j);
    rp[r] = v.x;
    tg[r] = v.y;
    uint64_t m = ((uint64_t)mhi << 32) | mlo;
    m &= m - 1ull;
    mlo = (uint32_t)m;
    mhi = (uint32_t)(m >> 32);
  }
}

// baseline/solvers.py:27-58 evaluated on the state, producing unit steps d (packed i16 pairs):
// availability 0 (fresh reset, or carrying) -> head for the own delivery target (the null cell
// after reset), else for the nearest open request by Manhattan distance, first (lowest pickup
// index) minimum wins; step = clip(goal - pos, -1, 1).  Random actions come from the
// POLICY/RANDOM streams.  Slots >= n get arbitrary steps: step_env never moves them.
// EFF: random moves are returned as the step they take (off-grid coordinates kept, core.py:282-287),
// so a step loop can add them without the clamp (step_env<CLAMP = false>); wh_policy reports the
// drawn action itself (EFF = false), as solvers.py:44-45 returns action_space.sample().
// WALKED: rp[] / tg[] hold the state's request walk already (policy_walk); else it is done here.
// EPS = false: the caller's p is 0 (the fused greedy rollout's eps = 0 instance): no random moves, and
// neither their code nor the test of p in the step loop.
template <class C, int POLICY, bool EFF = false, bool WALKED = false, bool EPS = true>
__device__ __forceinline__ void policy_steps(const Regs<C>& s, const Lds<C>& L, const Keys& k,
                                             uint32_t gid, float p, uint32_t (&d)[C::NAM],
                                             uint32_t (*walk_rp)[C::R] = nullptr,
                                             uint32_t (*walk_tg)[C::R] = nullptr) {
  const uint32_t t = s.hdr & 0xFFFFu;
  if (POLICY == POL_RANDOM) {
#pragma unroll
    for (int b = 0; b < (C::NAM + 3) / 4; ++b) {
      const uint4 blk = stream_block(k, gid, s.epi, t, PUR_RANDOM, (uint32_t)b);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int i = 4 * b + c;
        if (i < C::NAM) d[i] = L.mv(__umulhi(comp(blk, c), 9u));
      }
    }
  } else {
    WH_PHASE_MARK(policy_rtag);
    uint32_t rp[C::R], tg[C::R];
    if constexpr (WALKED) {
#pragma unroll
      for (int r = 0; r < C::R; ++r) {
        rp[r] = (*walk_rp)[r];
        tg[r] = (*walk_tg)[r];
      }
    } else {
      policy_walk<C>(s, L, rp, tg);
    }
    WH_PHASE_MARK(policy_agents);
#pragma unroll
    for (int i = 0; i < C::NAM; ++i) {
      const uint32_t a = s.ag[i];
      const uint32_t pos = a & XY16;
      uint32_t best = 0xFFFFFFFFu;
#pragma unroll
      for (int r = 0; r < C::R; ++r)   // key = dist << 16 | pickup << 10 | y << 5 | x
        best = min(best, __builtin_amdgcn_sad_hi_u8(pos, rp[r], tg[r]));
      const uint32_t near = (__builtin_amdgcn_ubfe(best, 5u, 5u) << 16) | (best & 31u);   // y << 16 | x
      const uint32_t dst = __builtin_amdgcn_perm(a, a, 0x0C030C01u);   // target bytes 1, 3 -> x | y << 16
      const uint32_t idle = (uint32_t)__builtin_amdgcn_sbfe((int)a, 15, 1);   // target byte 0xFF
      const uint32_t goal = msel(idle, near, dst);
      // goal is a grid cell, so pos + d stays on the grid: step_env<CLAMP = false> adds it as is
      d[i] = pk_min_i16(pk_max_i16(pk_sub_i16(goal, pos), 0xFFFFFFFFu), 0x00010001u);
    }
    if (EPS && WH_RARE(p > 0.0f)) {
#pragma unroll
      for (int b = 0; b < (C::NAM + 1) / 2; ++b) {
        const uint4 blk = stream_block(k, gid, s.epi, t, PUR_POLICY, (uint32_t)b);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int i = 2 * b + h;
          if (i < C::NAM) {
            const float u = (float)(comp(blk, 2 * h) >> 8) * (1.0f / 16777216.0f);
            uint32_t rnd = L.mv(__umulhi(comp(blk, 2 * h + 1), 9u));
            if (EFF) {
              const uint32_t pos = s.ag[i] & XY16;
              rnd = pk_sub_i16(step16<C::D>(pos, rnd), pos);
            }
            d[i] = (u < p) ? rnd : d[i];
          }
        }
      }
    }
  }
  // (slots >= n: whatever d says, step_env never moves them)
}
