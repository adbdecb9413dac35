// step_env.h -- one step of one env held in registers (device code; included by warehouse_amd.hip after
// device_vocab.h): step_env and its expiry and delivery phases, the image offsets of the observation values (obs_src), the reward-row
// writer (store_rewards) and assert mode's check_env.
// ----------------------------------------------------------------------------- step
// core.py:267-368 on one env held in registers.  Returns done.  No data-dependent branches:
// LDS side effects are predicated through neutral operands (and ~0 / or 0 / the scratch word),
// so each phase is one basic block and its LDS reads issue back to back.
// INJ = false compiles the injected-draw regeneration out (the fused rollout and the sampler step
// always draw from philox): less code in the step loop and no per-step test of `regen`.
// CLAMP = false: the steps come from the greedy policy, whose goals are grid cells, so pos + d
// never leaves the grid and the off-grid rule (a clamp) is the identity.
// rebuild and shared are wave-uniform (set from ballots, outside per-lane branches), so they live in
// scalar registers and the per-step tests of them are scalar compares: as per-lane flags each cost a
// v_cmp per step, and `rebuild` a register copy on the back-edge.
struct LazyGrid {
  bool rebuild;   // some lane's occupancy grid may lack an agent's cell: rebuild before the next move
  uint32_t cm;    // slots sharing a cell (found by the last rebuild): rebuild once one moves
  bool shared;    // some lane of the wave has such slots (cm != 0)
};

// What a launch's steps read of the env that only a reset changes, computed once and carried across
// the step loop's back-edge in registers (run_steps_fast; recomputed where a reset replaced n).
template <class C>
struct EnvConst {
  uint32_t live31[C::NAM];   // bit 31: slot i is live (i < n)
  uint32_t n16;              // n << 16, the header's agent-count field
  __device__ __forceinline__ void set(uint32_t hdr) {
    const uint32_t n = (hdr >> 16) & 0xFFu;
#pragma unroll
    for (int i = 0; i < C::NAM; ++i) live31[i] = (uint32_t)i - n;
    n16 = n << 16;
  }
};

#ifdef WH_COUNT_REV
__device__ unsigned long long g_wh_revcount[2];   // [0] reverse-key loops, [1] crossing-only loops
#endif

// The action-dict order of the ORDERED path: entry rows [B, ol] (ol = 1 .. 4 * NA: a dict may name an
// agent under each of its key forms) and the per-lane LDS key list of the entries' moves (16 bits
// each, [entry][lane]: OKeys, only in the ORDERED instances).
struct OrderIn {
  const int32_t* __restrict__ order;
  int ol;
  uint16_t* keys;
};
template <class C>
struct OKeys {
  uint16_t k[4 * C::NAM][BT];
};

// Request expiry (core.py:303-306), 4 pickup points per op.  Timer bytes hold the low 8 bits of the
// step at which the request expires (opened at t0 with wait W: t0 + W, the step whose decrement would
// reach 0), so nothing is decremented.  A request opened at t0 >= 0 cannot expire before step W, so
// waves with every t < W skip the phase (with T = W, 199 of 200 steps) unless they were loaded from a
// state outside that invariant (s.wskip).  Run before the move: expiry reads no positions and the
// move reads no requests, so the two commute, and the pickup table is final before the move loop --
// which lets its lookups be issued inside it.
template <class C>
__device__ __forceinline__ void expire_requests(Regs<C>& s, Lds<C>& L, uint32_t t, int tid, int ablate) {
  const uint64_t em = (ablate & 4) ? 0ull : __ballot(t >= s.wskip);
  if (WH_RARE(em != 0) && __popcll(em) == 1 && __ballot(true) == ~0ull) {
    // one lane of a full wave due (desynchronised episodes): its P pickup cells checked one per
    // lane of the wave, instead of the whole wave walking every lane's requests
    const int l = __builtin_ctzll(em), lane = tid & 63, col = (tid & ~63) + l;
    const uint32_t t8 = (uint32_t)__builtin_amdgcn_readlane(t, l) & 0xFFu;
    const uint32_t v = lane < C::P ? (uint32_t)L.pkp[lane][col] : 0u;
    const bool ex = (v & 0xFFu) != 0u && (v >> 8) == t8;
    if (ex) L.clear_target(lane, col);
    const uint64_t exm = __ballot(ex);
    s.am = lane == l ? (s.am & ~exm) : s.am;
  } else if (WH_RARE(em != 0)) {
    if (__any(__popcll(s.am) > C::R)) {   // a hand-built state with more than R requests: scan all
      uint64_t expired = 0;
#pragma unroll
      for (int j = 0; j < C::P; ++j) {
        const uint32_t v = L.pkp[j][tid];
        const bool ex = (v & 0xFFu) != 0u && (v >> 8) == (t & 0xFFu);
        if (ex) L.clear_target(j, tid);
        expired |= (uint64_t)ex << j;
      }
      s.am &= ~expired;
    } else {
      // walk the (at most R) open requests in the mask, as the policy does; index P (missing
      // slots) is the scratch row, and its "expiry" is discarded by the j < P test
      uint32_t mlo = (uint32_t)s.am, mhi = (uint32_t)(s.am >> 32), elo = 0, ehi = 0;
      const uint32_t t8 = t & 0xFFu;
#pragma unroll
      for (int r = 0; r < C::R; ++r) {
        uint32_t flo, fhi;
        asm("v_ffbl_b32 %0, %1" : "=v"(flo) : "v"(mlo));   // 0xFFFFFFFF when empty
        asm("v_ffbl_b32 %0, %1" : "=v"(fhi) : "v"(mhi));
        const uint32_t j = __builtin_elementwise_min(
            __builtin_elementwise_min(flo, __builtin_elementwise_add_sat(fhi, 32u)), (uint32_t)C::P);
        const uint32_t v = L.pkp[j][tid];
        const uint32_t ex = bop3<TA & TB>(mask_z((v >> 8) ^ t8), sgn(j - (uint32_t)C::P), 0xFFFFFFFFu);
        *reinterpret_cast<uint8_t*>(&L.pkp[msel(ex, j, (uint32_t)C::P)][tid]) = 0;
        const uint64_t b = 1ull << (j & 63u);
        elo |= bop3<TA & TB>(ex, (uint32_t)b, 0u);
        ehi |= bop3<TA & TB>(ex, (uint32_t)(b >> 32), 0u);
        uint64_t m = ((uint64_t)mhi << 32) | mlo;
        m &= m - 1ull;
        mlo = (uint32_t)m;
        mhi = (uint32_t)(m >> 32);
      }
      s.am &= ~(((uint64_t)ehi << 32) | elo);
    }
  }
}

// Deliveries (core.py:354-368): target cell == position (idle agents never match), and the step's
// rewards from the pickup masks (rewm) and the deliveries.
// Manhattan distance position -> target cell minus 1 is ONE v_sad_u8 of the agent word against its
// target bytes doubled ([x, dx, y, dy] vs [dx, dx, dy, dy], accumulator -1): negative exactly when the
// agent stands on its target (an idle agent's 0xFF bytes never match).  The reward of the pickup or
// the delivery is folded into the same bitop3 that makes the 1.0f.
template <class C>
__device__ __forceinline__ void deliver(Regs<C>& s, const uint32_t (&rewm)[C::NAM], float (&rew)[C::NAM], int ablate) {
  uint32_t delm[C::NAM];
#pragma unroll
  for (int i = 0; i < C::NAM; ++i) delm[i] = 0u;
  if (!(ablate & 32)) {
#pragma unroll
    for (int i = 0; i < C::NAM; ++i) {
      const uint32_t a = s.ag[i];
      const uint32_t m = sgn(__builtin_amdgcn_sad_u8(a, __builtin_amdgcn_perm(a, a, 0x03030101u), 0xFFFFFFFFu));
      s.ag[i] = bop3<(TA & TB) | TC>(m, IDLE, a);
      delm[i] = m;   // a pickup (interior cell) and a delivery (border cell) never share a step
    }
  }
#pragma unroll
  for (int i = 0; i < C::NAM; ++i) rew[i] = __uint_as_float(bop3<(TA | TB) & TC>(rewm[i], delm[i], 0x3F800000u));
}

template <class C, bool ORDERED, bool INJ = true, bool CLAMP = true, bool LAZY = false>
__device__ __forceinline__ bool step_env(Regs<C>& s, Lds<C>& L, const uint32_t (&dstep)[C::NAM],
                                         const OrderIn& oi,
                                         const int32_t* __restrict__ actions_g,
                                         const int32_t* __restrict__ regen, const Keys& k,
                                         uint32_t gid, int64_t e, int na, int phase, uint32_t T,
                                         uint32_t W, float (&rew)[C::NAM], int32_t* n_inactive,
                                         int tid, int ablate, LazyGrid* lg = nullptr,
                                         const uint4* pre_rblk = nullptr,
                                         const EnvConst<C>* ec = nullptr) {
  const uint32_t n = (s.hdr >> 16) & 0xFFu;
  uint32_t t = s.hdr & 0xFFFFu;
  uint32_t rewm[C::NAM];   // reward masks: all-ones = 1.0f
  // the regeneration's Philox block 0, where the caller computed it ahead of the policy (run_steps_fast)
  const uint4 rblk0 = pre_rblk ? *pre_rblk : make_uint4(0u, 0u, 0u, 0u);

  if (phase != PH_REGEN) {
    t = (t + 1u) & 0xFFFFu;                                 // core.py:267
#pragma unroll
    for (int i = 0; i < C::NAM; ++i) rewm[i] = 0u;

    WH_PHASE_MARK(expire);
    expire_requests<C>(s, L, t, tid, ablate);

    // ---- move + collision, sequential in action-dict order (core.py:275-300)
    // (This block and the regeneration stay in this body, unlike expiry and delivery.  Either one as a
    // __forceinline__ function of its own gave every k_step, k_sampler and k_step_record instance
    // another register allocation -- 18 of Medium-8's 39 kernels; the move block also +8/+9 v_mov_b32
    // and 74 more lines in the generic greedy k_step -- and nobody has timed those:
    // profiles/step_env_split_isa.txt.)
    WH_PHASE_MARK(move);
    uint32_t cp[C::NAM], tb[C::NAM], dst[C::NAM];   // pickup lookups (core.py:309-329): cell_row,
                                                    // target byte, delivery cell
    bool looked = false;
    // pickups (core.py:309-335): agent i takes iff it stands on a pickup point (cp != 0) with an
    // open request (tb != 0) and is idle -- slots >= n sit idle on the corner cell (0, 0), which is
    // no pickup point; min3 of the three 0/1-ish terms is 1 exactly when all hold.  Every agent
    // decides against the pre-pickup table (two agents on one point both take it), so the
    // points are cleared only after every agent's target byte has been read (clr[i]: the byte to
    // zero, row P = scratch).  The ascending move loop issues an agent's three dependent lookups
    // kPickDist turns apart and decides its pickup 3 * kPickDist turns after its move, when the
    // last lookup has landed, so only a few agents' lookups are live at a time.
    uint32_t prlo = 0, prhi = 0;   // points picked up, rotated left by one (see pick)
    uint32_t clr[C::NAM];
    auto pick = [&](int i, uint32_t cpv, uint32_t tbv, uint32_t dstv) {
      const uint32_t a = s.ag[i];
      const uint32_t idle01 = (a >> 15) & 1u;   // delivery-target byte 0xFF
      const uint32_t m = 0u - __builtin_elementwise_min(__builtin_elementwise_min(cpv, tbv), idle01);
      s.ag[i] = bop3<(TA & TB & TC) | (~TA & TB)>(m, a, dstv);   // idle target bytes are 0xFF
      // bit (j + 1) mod 64 for point j (cpv = j + 1): rotated back once after the loop
      const uint64_t bit = 1ull << (cpv & 63u);
      prlo = bop3<(TA & TB) | TC>(m, (uint32_t)bit, prlo);
      prhi = bop3<(TA & TB) | TC>(m, (uint32_t)(bit >> 32), prhi);
      clr[i] = msel(m, cpv, (uint32_t)(C::P + 1));
      rewm[i] = m;
    };
    if (!(ablate & 2)) {
      // The grid is rebuilt as {live agents' cells} (core.py:275-276) by OR-ing the cells into
      // what the previous step left, which is always a subset of them (a set bit is an arrival
      // or an agent that stayed; leaving clears), so no per-step clear is needed.  k_step clears
      // it at launch and after an auto-reset; the ordered (drop-in) path clears it every step.
      // LAZY (fused rollout): once rebuilt, the grid a lane carries stays exactly its agents' cells
      // (a move is accepted only into a free cell) until an agent leaves a cell it shares -- the
      // reference clears the cell under the agent that stays (core.py:290), and only its per-step
      // rebuild sets it again.  Shared cells come from resets, whose spawns are drawn independently
      // (core.py:191-201), and persist only while the agents sharing them stay put.  So a lane asks
      // for the rebuild (lg->rebuild) after a grid clear, and after a step in which an agent that
      // shares a cell (lg->cm) moved; the wave skips it when no lane asks.
      if (ORDERED) {
#pragma unroll
        for (int y = 0; y < C::D; ++y) L.occ[y][tid] = 0u;
      }
      if (!LAZY) {
#pragma unroll
        for (int i = 0; i < C::NAM; ++i) {
          const uint32_t p = s.ag[i] & XY16;
          const uint32_t mlive = sgn((uint32_t)i - n);
          atomicOr(&L.occ[p >> 16][tid], bop3<TA & TB>(mlive, 1u << (p & 31u), 0u));
        }
      } else if (WH_RARE(lg->rebuild)) {
        // (the terms are written so that none is shared with the move loop below: a shared one
        // would be hoisted above the branch, and the skip path would pay a register copy per term)
        const uint32_t livebits = (2u << (n - 1u)) - 1u;   // n >= 1
        uint32_t q[C::NAM];   // live cells; slots >= n get distinct off-grid stand-ins
#pragma unroll
        for (int i = 0; i < C::NAM; ++i) {
          const uint32_t a = s.ag[i];
          const uint32_t mlive = (uint32_t)__builtin_amdgcn_sbfe((int)livebits, (uint32_t)i, 1u);
          uint32_t bit;
          asm volatile("v_lshlrev_b32 %0, %1, 1" : "=v"(bit) : "v"(a));   // 1 << (x & 31)
          atomicOr(&L.occ[__builtin_amdgcn_ubfe(a, 16u, 8u)][tid], bop3<TA & TB>(mlive, bit, 0u));
          q[i] = msel(mlive, a, 0x80u + (uint32_t)i);   // position bytes compared below
        }
        uint32_t m[C::NAM];   // m[i] == 0: slot i shares its cell
#pragma unroll
        for (int i = 0; i < C::NAM; ++i) m[i] = 0xFFFFFFFFu;
#pragma unroll
        for (int i = 1; i < C::NAM; ++i)
#pragma unroll
          for (int j = 0; j < i; ++j) {
            const uint32_t x = bop3<(TA ^ TB) & TC>(q[i], q[j], XY16);
            m[i] = min(m[i], x);
            m[j] = min(m[j], x);
          }
        uint32_t cm = 0;
#pragma unroll
        for (int i = 0; i < C::NAM; ++i) cm |= (m[i] == 0u ? 1u : 0u) << i;
        lg->cm = cm;
        lg->shared = __any(cm != 0u);
        lg->rebuild = false;
      }
      if (ORDERED) {   // drop-in single env / BaseEnv: entries in action-dict order, records in LDS
        // Forbidden moves (core.py:293-297) by the ascending loop's one key per move (below): a move
        // p -> c is keyed by its direction and its undirected edge / square / cell
        // (u = p + c per coordinate), and an accepted move forbids exactly the moves with its u and
        // another direction (an accepted stay: every later stay on its cell, via a flipped low bit).
        // 16 bits per key: (dx + 1) | (dy + 1) << 2 | xsum << 4 | ysum << 10, so entry k is blocked iff
        // 1 <= (K_k ^ S_j) <= 15 for an earlier entry j; a rejected entry stores 0xFFFF (xsum 63:
        // never a real sum, D <= 32).  The keys live in LDS ([entry][lane]), so a dict of any length
        // up to 4 * NA entries runs in one pass: the first NAM entries unrolled (their order words
        // and key reads issued together), the rest -- only a dict naming agents under several keys
        // has them -- in a rolled loop.
#pragma unroll
        for (int i = 0; i < C::NAM; ++i) L.agl[i][tid] = s.ag[i];
        auto entry = [&](int sidx, int32_t raw, bool unrolled) {
          // entry: agent id in bits 0-7, optionally the entry's own action + 1 in bits 8-15 (a dict
          // naming one agent under several keys moves it once per key, with that key's action)
          int who = raw < 0 ? -1 : (raw & 0xFF);
          const uint32_t sact = raw < 0 ? 0u : ((uint32_t)raw >> 8) & 0xFFu;
          const bool live = who >= 0 && who < (int)n && who < C::NAM;
          who = live ? who : 0;
          const uint32_t a = L.agl[who][tid];
          const uint32_t mv = live ? (sact ? sact - 1u : (uint32_t)actions_g[e * na + who]) : 4u;
          const uint32_t p = a & XY16;
          const uint32_t c = step16<C::D>(p, L.mv(valid_action(mv)));
          const bool occupied = (L.occ[c >> 16][tid] >> (c & 31u)) & 1u;
          const uint32_t sum = as_u(as_s2(p) + as_s2(c)), dd = pk_sub_i16(c, p);
          const uint32_t key = (((dd + 1u) & 3u) | ((((dd >> 16) + 1u) & 3u) << 2) | ((sum & 63u) << 4) |
                                (((sum >> 16) & 63u) << 10));
          uint32_t f = 15u;
          if (unrolled) {
#pragma unroll
            for (int j = 0; j < C::NAM; ++j)
              if (j < sidx) f = min(f, (key ^ (uint32_t)oi.keys[j * BT + tid]) - 1u);
          } else {
            for (int j = 0; j < sidx; ++j) f = min(f, (key ^ (uint32_t)oi.keys[j * BT + tid]) - 1u);
          }
          const bool ok = live && !occupied && f >= 15u;
          atomicAnd(&L.occ[p >> 16][tid], ok ? ~(1u << (p & 31u)) : 0xFFFFFFFFu);
          atomicOr(&L.occ[c >> 16][tid], ok ? (1u << (c & 31u)) : 0u);
          oi.keys[sidx * BT + tid] = (uint16_t)(ok ? (dd == 0u ? key ^ 1u : key) : 0xFFFFu);
          L.agl[who][tid] = ok ? ((a & ~XY16) | c) : a;
        };
        const int32_t* orow = oi.order + e * oi.ol;
        int32_t raws[C::NAM];
#pragma unroll
        for (int sidx = 0; sidx < C::NAM; ++sidx) raws[sidx] = sidx < oi.ol ? orow[sidx] : -1;
#pragma unroll
        for (int sidx = 0; sidx < C::NAM; ++sidx) entry(sidx, raws[sidx], true);
        for (int sidx = C::NAM; sidx < oi.ol; ++sidx) entry(sidx, orow[sidx], false);
#pragma unroll
        for (int i = 0; i < C::NAM; ++i) s.ag[i] = L.agl[i][tid];
      } else {
        // Ascending agent order.  Every agent moves only on its own turn, so all candidate cells
        // are known up front.  The occupancy word for agent s+1 is read one turn early (before
        // agent s updates the grid) and corrected in registers for agent s's clear/set (4 VALU), so
        // the LDS latency -- which queues behind the turn's own lookups, lgkmcnt being in order --
        // is covered by a turn of work and no LDS round trip sits on the serial chain.  Reading two
        // turns early measured slower (Medium-8 +2.4 %, Large-16 +3.1 % per 200-step launch,
        // profiles/r05_occ_ab.txt: the second correction's VALU cost more than the wait it hid).
        // Agent s's pickup lookups (cell -> point, point -> target byte, target -> cell) are issued
        // kPickDist turns apart, from turn s on.
        // BIAS (greedy steps, never off the grid): positions carry the lane id in bits 8-15
        // (x | lane << 8 | y << 16), so `q >> 6` is the byte offset of the occupancy word
        // occ[y][lane] (y * 1024 + lane * 4; x < 32) -- one shift per LDS address instead of a
        // field extract and a shift-or.  Equality tests, x-bit selects and the move key's
        // coordinate sums are unaffected (every position of a lane carries the same lane bits).
        constexpr bool BIAS = !CLAMP;
        static_assert(BT * 4 == 1024 && C::D <= 32, "occ[y][lane] = byte y << 10 | lane << 2");
        const uint32_t lbias = BIAS ? ((uint32_t)tid & 255u) << 8 : 0u;
        auto occ_at = [&](uint32_t q) -> uint32_t* {
          if constexpr (BIAS)
            return reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(&L.occ[0][0]) + (q >> 6));
          else
            return &L.occ[q >> 16][tid];
        };
        uint32_t pp[C::NAM], cc[C::NAM];
#pragma unroll
        for (int i = 0; i < C::NAM; ++i) {
          pp[i] = (s.ag[i] & XY16) | lbias;
          cc[i] = CLAMP ? step16<C::D>(pp[i], dstep[i]) : as_u(as_s2(pp[i]) + as_s2(dstep[i]));
        }
        // Predicates are kept in bit 31 of VGPRs (x31 names) and selects are v_bitop3 with
        // 0 / all-ones masks (m names): no VCC round trips on the serial chain.
        //
        // Forbidden moves (core.py:293-297): the reverse of every accepted move, and for accepted
        // diagonals the two crossing moves.  One key per move and ONE test per earlier agent, exact
        // in every lane.  A unit move p -> c is keyed by its undirected edge or square, u = p + c
        // per coordinate (x and y sums; a stay has both even, an axis move one odd, a diagonal both
        // odd -- and both diagonals of a square share it), and by its direction (dx, dy) bytes:
        // K = dx | dy << 8 | xsum << 16 | ysum << 24.  The moves an accepted move forbids are
        // exactly those with its u and another direction -- its reverse, and for a diagonal the
        // two directions of the other diagonal -- so agent i is blocked iff some stored key S_j has
        // 1 <= (K_i ^ S_j) <= 0xFFFF: one v_xad ((K ^ S) - 1) and half a v_min3 per pair against a
        // cap of 0xFFFF.  An accepted stay adds its own key
        // (p, p) to the reference's set (it can be accepted where a co-located agent left the cell):
        // its stored key has the low bit flipped, so a later stay on that cell lands on 1.  A
        // rejected move stores ~0 (its high bytes never match: sums <= 62).  Same-box A/B against
        // the earlier two-key form (an ordered reverse key and a crossing-square key per move, the
        // reverse keys dropped for waves without co-located agents): 200-step launches Large-16
        // -10 %, Medium-8 -5 % (at Large that form made the step loop spill in its common path).
        // REV = false (a wave without co-located agents, below) stores every key as a stay's.
        uint32_t sk[C::NAM];
        auto move_loop = [&](auto rev_tag) {
          constexpr bool REV = decltype(rev_tag)::value;
          uint32_t raw = *occ_at(cc[0]);   // agent sidx's row word, read before agent sidx - 1's update
          uint32_t mokh[C::NAM];   // accept masks of the agents already moved
#pragma unroll
          for (int sidx = 0; sidx < C::NAM; ++sidx) {
            const uint32_t p = pp[sidx], c = cc[sidx], a = s.ag[sidx];
            // occupied: bit c of the row word, corrected for the clear-then-set of the agent that
            // moved after the word was read
            uint32_t occ31 = (uint32_t)__builtin_amdgcn_sbfe((int)raw, c, 1);
            if (sidx >= 1) {
              const int j = sidx - 1;
              const uint32_t set31 = (c ^ cc[j]) - 1u;   // bit 31: c == agent j's new cell
              const uint32_t clr31 = (c ^ pp[j]) - 1u;   // bit 31: c == agent j's old cell
              occ31 = bop3<(TA & TB) | (TC & ~(TA & TB))>(mokh[j], set31, bop3<TC & ~(TA & TB)>(mokh[j], clr31, occ31));
            }
            // agent sidx + 1's word, before this turn's update
            if (sidx + 1 < C::NAM) raw = *occ_at(cc[sidx + 1 < C::NAM ? sidx + 1 : 0]);
            const uint32_t dd = CLAMP ? pk_sub_i16(c, p) : dstep[sidx];
            const uint32_t kpr = __builtin_amdgcn_perm(as_u(as_s2(p) + as_s2(c)), dd, 0x06040200u);
            uint32_t f = 0xFFFFu;
#pragma unroll
            for (int j = 0; j < sidx; ++j) f = min(f, (kpr ^ sk[j]) - 1u);
            f -= 0xFFFEu;   // bit 31 of f - 1 below: blocked (f was < 0xFFFF)
            const uint32_t live31 = ec ? ec->live31[sidx] : (uint32_t)sidx - n;   // bit 31: sidx < n
            const uint32_t mok = sgn(bop3<TA & ~TB & ~TC>(live31, occ31, f - 1u));
            atomicAnd(occ_at(p), bop3<~(TA & TB)>(mok, 1u << (p & 31u), 0u));
            atomicOr(occ_at(c), bop3<TA & TB>(mok, 1u << (c & 31u), 0u));
            const uint32_t dxy = c ^ p;
            if constexpr (REV) {
              uint32_t z;   // 1 for a stay: v_ffbl of 0 is ~0
              asm("v_ffbl_b32 %0, %1" : "=v"(z) : "v"(dd));
              sk[sidx] = bop3<~TA | (TB ^ TC)>(mok, kpr, z >> 31);
            } else {
              // No lane of the wave has co-located agents: a later agent can then never make the
              // same move p -> c as an accepted one (it would have to stand on p too), so every
              // stored key may carry the flipped low bit a stay's needs -- one op instead of three
              sk[sidx] = bop3<~TA | (TB ^ TC)>(mok, kpr, 1u);
            }
            const uint32_t moved = bop3<TA ^ (TB & TC)>(a, mok, dxy);
            s.ag[sidx] = moved;
            mokh[sidx] = mok;
            constexpr int PD = kPickDist;
            cp[sidx] = L.cell_row(moved);
            if (sidx >= PD) tb[sidx - PD] = L.row_target(cp[sidx >= PD ? sidx - PD : 0], tid);
            if (sidx >= 2 * PD) dst[sidx - 2 * PD] = L.dst_tb(tb[sidx >= 2 * PD ? sidx - 2 * PD : 0]);
            if (!(ablate & 8) && sidx >= 3 * PD) {
              const int j = sidx >= 3 * PD ? sidx - 3 * PD : 0;
              pick(j, cp[j], tb[j], dst[j]);
            }
          }
        };
        // did an agent that shares a cell move?  (positions are final after the move loop: a pickup
        // changes target bytes only)
        auto shared_moved = [&]() {
          uint32_t acc = 0;
#pragma unroll
          for (int i = 0; i < C::NAM; ++i)
            acc |= (s.ag[i] ^ pp[i]) & (XY16 & (uint32_t)__builtin_amdgcn_sbfe((int)lg->cm, (uint32_t)i, 1u));
          lg->rebuild = lg->rebuild || __any(acc != 0u);
        };
        // Where the reverse-key loop runs exactly for the waves with shared cells, that test is made
        // on its (rare) side of the branch, so the common path has no branch between the pickup
        // tail and regeneration item 0 and the two are scheduled as one block.
        constexpr bool CM_IN_REV = LAZY && C::NAM <= kRevSplitMaxNam;
        // REV: the exact loop for waves with co-located agents (only a stay's key flipped), else the
        // loop for waves without any (every key flipped).  The lazy grid knows the lanes with shared
        // cells (lg->cm, from the last rebuild; new sharing needs an existing one).  From
        // kRevSplitMaxNam agents on a single (exact) loop.
        if (!LAZY || C::NAM > kRevSplitMaxNam || WH_RARE(lg->shared)) {
#ifdef WH_COUNT_REV   // A/B builds: count the wave-steps that take the reverse-key loop (wh_check_read)
          if (LAZY && __lane_id() == 0) atomicAdd(&g_wh_revcount[0], 1ull);
#endif
          move_loop(std::true_type{});
          if constexpr (CM_IN_REV) shared_moved();
        } else {
#ifdef WH_COUNT_REV
          if (__lane_id() == 0) atomicAdd(&g_wh_revcount[1], 1ull);
#endif
          move_loop(std::false_type{});
        }
        // the lookups and decisions the loop's last turns did not reach, in dependency order
        constexpr int PD = kPickDist;
#pragma unroll
        for (int i = (C::NAM > PD ? C::NAM - PD : 0); i < C::NAM; ++i) tb[i] = L.row_target(cp[i], tid);
#pragma unroll
        for (int i = (C::NAM > 2 * PD ? C::NAM - 2 * PD : 0); i < C::NAM; ++i) dst[i] = L.dst_tb(tb[i]);
        if (!(ablate & 8)) {
#pragma unroll
          for (int i = (C::NAM > 3 * PD ? C::NAM - 3 * PD : 0); i < C::NAM; ++i) pick(i, cp[i], tb[i], dst[i]);
        }
        looked = true;
        if constexpr (LAZY && !CM_IN_REV) {
          if (WH_RARE(lg->shared)) shared_moved();
        }
      }
    }

    // ---- pickups: every agent decided against the pre-pickup table, then the table is cleared
    //      (core.py:309-335; two agents on one point both pick it up)
    WH_PHASE_MARK(pickup);
    if (!(ablate & 8)) {
      if (!looked) {
#pragma unroll
        for (int i = 0; i < C::NAM; ++i) cp[i] = L.cell_row(s.ag[i]);
#pragma unroll
        for (int i = 0; i < C::NAM; ++i) tb[i] = L.row_target(cp[i], tid);
#pragma unroll
        for (int i = 0; i < C::NAM; ++i) dst[i] = L.dst_tb(tb[i]);
#pragma unroll
        for (int i = 0; i < C::NAM; ++i) pick(i, cp[i], tb[i], dst[i]);
      }
#pragma unroll
      for (int i = 0; i < C::NAM; ++i) *L.row_byte(clr[i], tid) = 0;
      const uint64_t pr = ((uint64_t)prhi << 32) | prlo;
      s.am &= ~((pr >> 1) | (pr << 63));
    }
  }

  // ---- regeneration: reopen k = R - P + |inactive| points (core.py:338-351)
  WH_PHASE_MARK(regen);
  if (!(ablate & 16)) {
    const uint64_t inactive = ~s.am & low_mask<C::P>();
    const uint32_t nin = (uint32_t)__popcll(inactive);
    // The fused rollout (INJ = false) always auto-resets a finished episode, and a regeneration
    // at its last step (t = T) lands in state the reset replaces: skipped.  (With desynchronised
    // episodes that step's expiry makes it the deepest regeneration of the episode, and the whole
    // wave would walk it for one lane.)
    const int kreq = (!INJ && t >= T) ? 0 : C::R - C::P + (int)nin;
    if (phase == PH_PRE) {
      if (n_inactive) n_inactive[e] = (int32_t)nin;
    } else {
      // 64-bit sets as (lo, hi) halves so that every mask consumer is a v_bitop3
      uint32_t rlo = (uint32_t)inactive, rhi = (uint32_t)(inactive >> 32);   // still selectable
      uint32_t ulo = 0, uhi = 0;                                               // targets used
      uint32_t olo = 0, ohi = 0;                                               // points opened
      // Targets of items 1 and 2 by skipping the earlier items' targets (a compare-add each) instead
      // of a rank selection on a used-target mask; the mask is built only from item 3 on.  Same values.
      uint32_t tj[3] = {0u, 0u, 0u};   // targets of items 0-2
      uint32_t first_t = 0;
      const uint32_t wexp = ((t + W) & 0xFFu) << 8;   // expires at step t + W
      uint4 blk = make_uint4(0u, 0u, 0u, 0u);   // words 2j (pickup) and 2j+1 (target) share a block
#pragma unroll
      for (int j = 0; j < C::R; ++j) {
        // wave-uniform: once no env needs item j, none needs a later one -- leave the loop (one
        // branch test per executed item + 1, instead of one per item)
        if (!__any(j < kreq)) break;
        {
          uint32_t ma = sgn((uint32_t)j - (uint32_t)kreq);   // j < kreq
          uint32_t sel, tgi;
          if (INJ && regen) {
            const uint32_t rpos = (uint32_t)regen[e * 2 * C::R + j];
            tgi = (uint32_t)regen[e * 2 * C::R + C::R + j];
            const bool valid = rpos < nin && tgi < (uint32_t)C::DP;   // invalid draws are ignored
            ma = bop3<TA & TB>(ma, 0u - (uint32_t)valid, 0u);
            sel = select_bit64(inactive, rpos);   // positions into the inactive list, host-drawn
          } else {
            if ((j & 1) == 0) blk = (j == 0 && pre_rblk) ? rblk0 : stream_block(k, gid, s.epi, t, PUR_REGEN, (uint32_t)(j >> 1));
            const uint32_t w1 = comp(blk, (2 * j) & 3), w2 = comp(blk, (2 * j + 1) & 3);
            sel = select_bit64(((uint64_t)rhi << 32) | rlo, __umulhi(w1, nin - (uint32_t)j));
            const uint32_t r2 = __umulhi(w2, (uint32_t)(C::DP - j));
            if (j == 0) tgi = r2;                                               // nothing used yet
            else if (j == 1) tgi = r2 + ((first_t - 1u - r2) >> 31);   // + (r2 >= first): skip it
            else if (j == 2) {
              // the r2-th target not used by items 0 and 1: skip each of them at or below it, in
              // ascending order (the same value as the rank selection on the used mask)
              const uint32_t lo = min(tj[0], tj[1]), hi = max(tj[0], tj[1]);
              tgi = r2 + ((lo - 1u - r2) >> 31);
              tgi += (hi - 1u - tgi) >> 31;
            } else {
              if (j == 3) {   // from item 3 on: the used mask, built from items 0-2
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                  const uint64_t b = 1ull << (tj[q] & 63u);
                  ulo |= (uint32_t)b;
                  uhi |= (uint32_t)(b >> 32);
                }
              }
              tgi = select_bit64(~(((uint64_t)uhi << 32) | ulo) & low_mask<C::DP>(), r2);
            }
            if (j == 0) first_t = r2;
            if (j < 3) tj[j] = tgi;
          }
          const uint64_t sb = 1ull << (sel & 63u), tb64 = 1ull << (tgi & 63u);
          const uint32_t slo = bop3<TA & TB>(ma, (uint32_t)sb, 0u), shi = bop3<TA & TB>(ma, (uint32_t)(sb >> 32), 0u);
          rlo &= ~slo;
          rhi &= ~shi;
          olo |= slo;
          ohi |= shi;
          if (j >= 3) {   // (items 0-2 skip their targets arithmetically)
            ulo = bop3<(TA & TB) | TC>(ma, (uint32_t)tb64, ulo);
            uhi = bop3<(TA & TB) | TC>(ma, (uint32_t)(tb64 >> 32), uhi);
          }
          // predicated store: lanes with nothing to open write the scratch row
          L.pkp[msel(ma, sel, (uint32_t)C::P)][tid] = (uint16_t)((tgi + 1u) | wexp);
        }
      }
      const uint64_t opened = ((uint64_t)ohi << 32) | olo;
      s.am |= opened;
    }
  }

  bool done = false;
  if (phase != PH_REGEN) {
    WH_PHASE_MARK(deliver);
    deliver<C>(s, rewm, rew, ablate);
    WH_PHASE_MARK(tail);
    done = t >= T;                                            // core.py:438
    s.hdr = t | (ec ? ec->n16 : n << 16);                     // clears `fresh`
  }
  return done;
}

// The fused rollout's step (FastRun::step, run_steps_fast): every agent slot in ascending order, all
// phases, Philox regeneration, the lazy grid; rb and ec may be null (step_env).
template <class C, bool CLAMP>
__device__ __forceinline__ bool step_env_fused(Regs<C>& s, Lds<C>& L, const uint32_t (&dstep)[C::NAM], const Keys& k,
                                               uint32_t gid, int64_t e, uint32_t T, uint32_t W, float (&rew)[C::NAM],
                                               int tid, int ablate, LazyGrid* lg, const uint4* rb,
                                               const EnvConst<C>* ec) {
  return step_env<C, false, false, CLAMP, true>(s, L, dstep, OrderIn{nullptr, 0, nullptr}, nullptr, nullptr, k, gid, e,
                                                C::NAM, PH_ALL, T, W, rew, nullptr, tid, ablate, lg, rb, ec);
}

// Image offset of output value f of agent row i (sorted-key order, see wh_observe).
// Image layout: [0] n, [A0 + r] availability of agent r, [G0 + 2r] its delivery target (x, y),
// [P0 + 2r] its position (x, y), [Q0 + 4q] request q (pickup x, y, delivery x, y); k_observe's
// byte image packs the sections back to back (the defaults).
template <int R, int A0 = 1, int G0 = 1 + R, int P0 = 1 + 3 * R, int Q0 = 1 + 5 * R>
__host__ __device__ constexpr uint32_t obs_src(int i, int f, bool fresh) {
  if (f == 0) return 0;                                                    // num_agents
  if (f < R) {                                                             // other_availabilities
    const int j = f - 1;
    return A0 + (j < i ? j : j + 1);
  }
  if (f < 3 * R - 2) {                                                     // other_delivery_targets
    const int k = f - R, j = k >> 1, drop = fresh ? i : 1;
    return G0 + 2 * (j < drop ? j : j + 1) + (k & 1);
  }
  if (f < 5 * R - 4) {                                                     // other_positions
    const int k = f - (3 * R - 2), j = k >> 1;
    return P0 + 2 * (j < i ? j : j + 1) + (k & 1);
  }
  if (f < 9 * R - 4) return Q0 + (f - (5 * R - 4));                        // requests
  if (f == 9 * R - 4) return A0 + i;                                       // self_availability
  if (f < 9 * R - 1) return G0 + 2 * i + (f - (9 * R - 3));                // self_delivery_target
  return P0 + 2 * i + (f - (9 * R - 1));                                   // self_position
}

// ----------------------------------------------------------------------------- kernels
// rewards[B, na]: a wave's 64 envs own one contiguous block of 64*na floats.  Even agent counts
// store each lane's row with 16/8-byte stores; otherwise lanes write their rows into LDS (the agl
// scratch, free after the move phase) and read the block back so every global store instruction
// writes contiguous 16-byte lanes instead of one strided row per lane.
// One env's row of an even agent count (16- or 8-byte aligned) as 16-byte (8-byte) stores.
template <class C>
__device__ __forceinline__ void store_row(float* row, const float (&rew)[C::NAM]) {
  if constexpr ((C::NAM & 3) == 0) {
#pragma unroll
    for (int q = 0; q < C::NAM / 4; ++q)
      reinterpret_cast<float4*>(row)[q] = make_float4(rew[4 * q], rew[4 * q + 1], rew[4 * q + 2], rew[4 * q + 3]);
  } else {
#pragma unroll
    for (int q = 0; q < C::NAM / 2; ++q) reinterpret_cast<float2*>(row)[q] = make_float2(rew[2 * q], rew[2 * q + 1]);
  }
}

template <class C>
__device__ __forceinline__ void store_rewards(Lds<C>& L, const float (&rew)[C::NAM], float* out,
                                              int64_t B, int64_t e, int na, int tid, bool direct) {
  if ((C::NAM & 1) == 0 && na == C::NAM && (reinterpret_cast<uintptr_t>(out) & 15u) == 0) {
    // One row of 16-byte (8-byte) stores per lane: the two wave-instructions of a Medium-8 step
    // cover the wave's contiguous 2 KiB block between them (A/B: 5 % faster than the LDS transpose
    // below, whose row writes are 8-way bank conflicts).
    store_row<C>(out + e * na, rew);
    return;
  }
  const int lane = tid & 63;
  const int64_t e0 = e - lane;
  // tail wave (lanes past B have exited) or masked step (unstepped lanes have exited): no
  // transpose -- one row per lane
  if (direct || B - e0 < 64) {
    float* row = out + e * na;
#pragma unroll
    for (int i = 0; i < C::NAM; ++i)
      if (i < na) row[i] = rew[i];
    return;
  }
  // Staging element k of this wave's 64*na floats lives at agl[k / 64][wave base + k % 64]: inside
  // the wave's own columns, so no other wave's agent words (ordered path) are overwritten.
  const int wbase = tid & ~63;
  auto stg = [&](int k) -> float* { return reinterpret_cast<float*>(&L.agl[k >> 6][wbase + (k & 63)]); };
#pragma unroll
  for (int i = 0; i < C::NAM; ++i)
    if (i < na) *stg(lane * na + i) = rew[i];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int nvalid = 64 * na;
  float* wout = out + e0 * na;
  if ((reinterpret_cast<uintptr_t>(wout) & 15u) == 0 && (na & 3) == 0) {
#pragma unroll
    for (int q = 0; q < C::NAM / 4; ++q)
      if (4 * q < na)   // 4 consecutive k (k % 4 == 0) sit in one row, 16-byte aligned
        reinterpret_cast<float4*>(wout)[lane + 64 * q] = *reinterpret_cast<const float4*>(stg(4 * (lane + 64 * q)));
  } else {
#pragma unroll
    for (int q = 0; q < C::NAM; ++q)
      if (lane + 64 * q < nvalid) wout[lane + 64 * q] = *stg(lane + 64 * q);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// ----------------------------------------------------------------------------- assert mode
// -DWH_CHECK builds verify SURVEY §5's invariants in the kernel after the state load and after
// every step (and auto-reset): exactly R open requests (core.py:210-221 opens R, core.py:338-351
// refills to R), every live agent inside the grid, every carried target a delivery cell
// (core.py:177-188), every request byte a valid delivery index, the open-request mask equal to the
// table, n <= agent slots.  Violations are counted in g_wh_check (read by wh_check_read): [0]
// violations, [1] first failing env id, [2] its bit mask of failed checks, [3] env-states checked.
#ifdef WH_CHECK
__device__ unsigned long long g_wh_check[4];

template <class C>
__device__ __forceinline__ void check_env(const Regs<C>& s, const Lds<C>& L, int64_t e, int tid) {
  const uint32_t n = (s.hdr >> 16) & 0xFFu;
  uint32_t code = 0;
  if (n > (uint32_t)C::NAM) code |= 1u;
  if (__popcll(s.am) != C::R) code |= 2u;
#pragma unroll
  for (int i = 0; i < C::NAM; ++i) {
    if ((uint32_t)i >= n) continue;
    const uint32_t a = s.ag[i];
    const uint32_t x = a & 0xFFu, y = (a >> 16) & 0xFFu, dx = (a >> 8) & 0xFFu, dy = a >> 24;
    if (x >= (uint32_t)C::D || y >= (uint32_t)C::D) code |= 4u;
    if ((dx == 0xFFu) != (dy == 0xFFu)) code |= 8u;
    if (dx != 0xFFu) {
      const bool xb = dx == 0u || dx == (uint32_t)(C::D - 1), yb = dy == 0u || dy == (uint32_t)(C::D - 1);
      const bool ok = (xb && !yb && dy >= 2u && dy <= (uint32_t)(C::D - 3)) ||
                      (yb && !xb && dx >= 2u && dx <= (uint32_t)(C::D - 3));
      if (!ok) code |= 8u;
    }
  }
#pragma unroll
  for (int j = 0; j < C::P; ++j) {
    const uint32_t tb = L.pkp[j][tid] & 0xFFu;
    if ((tb != 0u) != (((s.am >> j) & 1ull) != 0ull)) code |= 16u;
    if (tb > (uint32_t)C::DP) code |= 32u;
  }
  if (code) {
    if (atomicAdd(&g_wh_check[0], 1ull) == 0ull) {
      g_wh_check[1] = (unsigned long long)e;
      g_wh_check[2] = code;
    }
  }
}
#define WH_CHECK_ENV(s, L, e, tid) check_env<C>(s, L, e, tid)
#else
#define WH_CHECK_ENV(s, L, e, tid) ((void)0)
#endif
