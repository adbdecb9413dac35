// step_wide.h -- the 16-lanes-per-env form of the step (device code; included by warehouse_amd.hip
// after StepParams and flush_episodes).
//
// One env is spread over a group of WH_WIDE_LANES = 16 lanes -- one DPP row, so row-scoped
// cross-lane operations (row_newbcast, row_ror) and width-16 shuffles stay inside an env.  A wave
// holds 4 envs, a 256-lane workgroup 16.  Below one wave per SIMD the lane-per-env kernels' step
// latency is one lane's serial walk over its env's agents and pickup words; here
//   * lane l holds agent word l (l < n) and, for l < P/4, packed request-target word l and expiry
//     word l, so expiry, pickups, deliveries and the state load/store are one pass for all agents
//     and all points;
//   * the header fields (t, n, fresh, episode) and the 64-bit open-request mask are kept
//     group-uniform (every lane of the group holds the same value), so rank selections and the
//     regeneration run redundantly in every lane and only the owning lane applies a result;
//   * occupancy is a real D x D bit grid, cell c = y * D + x held in lane c >> 5, rebuilt every
//     step (core.py:275-276): an agent leaving a shared cell clears it under the agent that stays;
//   * the move loop stays serial over agents (core.py:279-300), but a turn is one row broadcast of
//     that agent's precomputed (from, to) cells and move key, one test per lane (its grid word,
//     its own invalid-move keys) and a group-scoped any;
//   * a Philox stream never needs more than 16 blocks per event, so lane b computes block b and
//     the words are shuffled out.
// It is a port of csrc/host_engine.cpp (load/store, reset_philox, move_phase, expiry / pickup /
// regenerate / delivery, policy_env): the same transitions, draws and packed state, bit for bit.
// All 64 lanes of a wave stay converged through every cross-lane operation: groups past B or
// masked out run on a copy of a real env and write nothing.

constexpr int WL = WH_WIDE_LANES;
constexpr int WIDE_ENVS = BT / WL;   // envs per workgroup
static_assert(WL == 16, "a group is one DPP row");

template <class C>
struct WideLds {
  alignas(16) uint32_t tbl[4 * C::TBL4];   // the geometry tables (TableLayout)
};

// lane I of the row to every lane of the row / the row rotated by N lanes (full-rate DPP moves)
template <int I>
__device__ __forceinline__ uint32_t row_bcast(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x150 + I, 0xF, 0xF, false);
}
template <int N>
__device__ __forceinline__ uint32_t row_ror(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x120 + N, 0xF, 0xF, false);
}
// OR over the 16 lanes of the row, in every lane
__device__ __forceinline__ uint32_t row_or(uint32_t v) {
  v |= row_ror<8>(v);
  v |= row_ror<4>(v);
  v |= row_ror<2>(v);
  v |= row_ror<1>(v);
  return v;
}
__device__ __forceinline__ uint64_t row_or64(uint64_t v) {
  return ((uint64_t)row_or((uint32_t)(v >> 32)) << 32) | row_or((uint32_t)v);
}
// lane `src` (0..15) of the own group
__device__ __forceinline__ uint32_t grp_get(uint32_t v, uint32_t src) { return (uint32_t)__shfl((int)v, (int)src, WL); }

// word idx of the group's Philox stream (lane b holds block b).  _u: idx is the same in every lane
// of the group (the source lane picks the component); _v: idx differs per lane.
__device__ __forceinline__ uint32_t grp_word_u(const uint4& blk, uint32_t idx) {
  return grp_get(comp(blk, (int)(idx & 3u)), idx >> 2);
}
__device__ __forceinline__ uint32_t grp_word_v(const uint4& blk, uint32_t idx) {
  const uint32_t s = idx >> 2;
  const uint4 v = make_uint4(grp_get(blk.x, s), grp_get(blk.y, s), grp_get(blk.z, s), grp_get(blk.w, s));
  return comp(v, (int)(idx & 3u));
}

// Group-uniform part of one env plus lane l's agent word and pickup words.
struct WideEnv {
  uint32_t t, n, fresh, epi;   // group-uniform
  uint32_t ag;                 // agent l (IDLE at (0,0) for l >= n)
  uint32_t pt, pe;             // request-target bytes / expiry bytes of points 4l .. 4l+3 (0 for l >= P/4)
  uint64_t am;                 // open requests, group-uniform
};

// bit j = point j has a request, from the lanes' target words
__device__ __forceinline__ uint64_t wide_open_mask(uint32_t pt, uint32_t l) {
  return row_or64((uint64_t)nib_of(nz_hi(pt)) << (4u * l));
}

template <class C>
__device__ __forceinline__ void wide_set_request(WideEnv& s, uint32_t l, bool on, uint32_t sel, uint32_t tgi, uint32_t exp) {
  if (on && (sel >> 2) == l) {
    const uint32_t sh = 8u * (sel & 3u);
    s.pt = (s.pt & ~(0xFFu << sh)) | ((tgi + 1u) << sh);
    s.pe = (s.pe & ~(0xFFu << sh)) | (exp << sh);
  }
}

// host_engine.cpp reset_philox: RESET stream of episode epi + 1 at t = 0; word 0 the agent count,
// words 1..NA the spawn cells, then (point, target) per request.  Returns the new env; the caller
// keeps it for the groups whose episode ended.
template <class C>
__device__ __forceinline__ WideEnv wide_reset(const WideEnv& s, const uint32_t* tbl, const Keys& k, uint32_t gid,
                                              uint32_t l, int na, int variable_n, uint32_t W) {
  WideEnv r;
  const uint32_t ep = s.epi + 1u;
  const uint4 blk = stream_block(k, gid, ep, 0u, PUR_RESET, l);
  const uint32_t n = variable_n ? 1u + __umulhi(grp_word_u(blk, 0u), (uint32_t)na) : (uint32_t)na;
  const uint32_t wv = grp_word_v(blk, 1u + min(l, (uint32_t)na - 1u));
  const uint32_t cell = tbl[C::T.valid / 4 + __umulhi(wv, (uint32_t)C::NV)];   // x | y << 16
  r.ag = l < n ? (cell | IDLE) : IDLE;
  uint64_t taken = 0, used = 0;
  uint32_t pt = 0, pe = 0;
  for (int j = 0; j < C::R; ++j) {
    const uint32_t m = (uint32_t)(C::P - C::R + j);
    const uint32_t rr = __umulhi(grp_word_u(blk, (uint32_t)(1 + na + 2 * j)), m + 1u);
    const uint32_t sel = (j > 0 && ((taken >> rr) & 1ull)) ? m : rr;   // Floyd's subset
    taken |= 1ull << sel;
    const uint32_t rank = __umulhi(grp_word_u(blk, (uint32_t)(2 + na + 2 * j)), (uint32_t)(C::DP - j));
    const uint32_t d = select_bit64(~used & low_mask<C::DP>(), rank);   // the rank-th unused target
    used |= 1ull << d;
    if ((sel >> 2) == l) {
      pt |= (d + 1u) << (8u * (sel & 3u));
      pe |= (W & 0xFFu) << (8u * (sel & 3u));
    }
  }
  r.pt = pt;
  r.pe = pe;
  r.am = taken;
  r.t = 0u;
  r.n = n;
  r.fresh = 1u;
  r.epi = ep;
  return r;
}

// host_engine.cpp policy_env for agent l: the action index 0..8 (4 for l >= n).
template <class C, int POLICY>
__device__ __forceinline__ uint32_t wide_policy(const WideEnv& s, const uint32_t* tbl, const Keys& k, uint32_t gid,
                                                uint32_t l, float p) {
  uint32_t act = 4u;
  if (POLICY == POL_RANDOM) {
    const uint4 blk = stream_block(k, gid, s.epi, s.t, PUR_RANDOM, l >> 2);   // word l
    if (l < s.n) act = __umulhi(comp(blk, (int)(l & 3u)), 9u);
    return act;
  }
  const int x = (int)(s.ag & 0xFFu), y = (int)((s.ag >> 16) & 0xFFu);
  int gx = C::D / 2, gy = C::D / 2;   // the null cell: fresh resets head there (core.py:233-236)
  const uint32_t dx = (s.ag >> 8) & 0xFFu;
  if (!s.fresh) {
    if (dx != 0xFFu) {
      gx = (int)dx;
      gy = (int)(s.ag >> 24);
    } else {
      // nearest open request, first minimum = lowest point index (solvers.py:53-58): the open set
      // is group-uniform, so every agent lane walks the same <= R points
      int best = 1 << 30;
      uint64_t m = s.am;
      while (m) {
        const int j = __ffsll((unsigned long long)m) - 1;
        m &= m - 1ull;
        const uint32_t rp = tbl[C::T.rp / 4 + 2 * j];   // x | y << 16
        const int qx = (int)(rp & 0xFFFFu), qy = (int)(rp >> 16);
        const int dist = abs(qx - x) + abs(qy - y);
        if (dist < best) {
          best = dist;
          gx = qx;
          gy = qy;
        }
      }
    }
  }
  const int sx = max(-1, min(1, gx - x)), sy = max(-1, min(1, gy - y));
  uint32_t a = (uint32_t)((sx + 1) * 3 + (sy + 1));
  if (p > 0.0f) {   // POLICY stream: word 2l the coin, 2l + 1 the move
    const uint4 blk = stream_block(k, gid, s.epi, s.t, PUR_POLICY, l >> 1);
    const uint32_t coin = (l & 1u) ? blk.z : blk.x, mv = (l & 1u) ? blk.w : blk.y;
    const float u = (float)(coin >> 8) * (1.0f / 16777216.0f);
    if (u < p) a = __umulhi(mv, 9u);
  }
  if (l < s.n) act = a;
  return act;
}

// One transition (host_engine.cpp step_env, PHASE_ALL, ascending order).  `act` is lane l's action;
// gmask the 64-bit ballot mask of the lane's group.  Returns lane l's reward flag; done / nin out.
template <class C>
__device__ __forceinline__ bool wide_step(WideEnv& s, const uint32_t* tbl, const Keys& k, uint32_t gid, uint32_t l,
                                          uint64_t gmask, uint32_t act, const int32_t* regen, bool skip_regen_if_done,
                                          uint32_t T, uint32_t W, bool& done, uint32_t& nin_out) {
  constexpr int D = C::D;
  static_assert(D * D <= 32 * WL, "the bit grid fits one word per lane");
  s.t = (s.t + 1u) & 0xFFFFu;                                        // core.py:267
  const uint32_t n = s.n;
  // ---- moves (core.py:275-300).  Every agent's from/to cells and move key are known up front:
  // only whether the move is accepted depends on the agents before it.
  if (act > 8u) act = 4u;
  const int x = (int)(s.ag & 0xFFu), y = (int)((s.ag >> 16) & 0xFFu);
  int tx = x + (int)(act / 3u) - 1, ty = y + (int)(act % 3u) - 1;
  if (!(0 <= tx && tx < D)) tx = x;                                  // core.py:284-287
  if (!(0 <= ty && ty < D)) ty = y;
  const uint32_t ux = (uint32_t)x, uy = (uint32_t)y, utx = (uint32_t)tx, uty = (uint32_t)ty;
  const uint32_t cc = (uy * D + ux) | ((uty * D + utx) << 16);       // from cell | to cell << 16
  const uint32_t key = ux | (uy << 8) | (utx << 16) | (uty << 24);   // (from, to)
  // the invalid-move keys this agent's accepted move produces (core.py:293-297)
  const bool diag = tx != x && ty != y;
  const uint32_t kr = utx | (uty << 8) | (ux << 16) | (uy << 24);
  const uint32_t kd1 = diag ? (utx | (uy << 8) | (ux << 16) | (uty << 24)) : 0xFFFFFFFFu;
  const uint32_t kd2 = diag ? (ux | (uty << 8) | (utx << 16) | (uy << 24)) : 0xFFFFFFFFu;
  uint32_t cci[C::NAM], kki[C::NAM];
  {
    // (a constexpr-indexed unroll: row_bcast's lane is an immediate)
    auto fill = [&](auto self, auto ic) -> void {
      constexpr int i = decltype(ic)::value;
      if constexpr (i < C::NAM) {
        cci[i] = row_bcast<i>(cc);
        kki[i] = row_bcast<i>(key);
        self(self, std::integral_constant<int, i + 1>{});
      }
    };
    fill(fill, std::integral_constant<int, 0>{});
  }
  uint32_t occw = 0;   // bit (c & 31) of lane c >> 5: cell c occupied
#pragma unroll
  for (int i = 0; i < C::NAM; ++i) {
    const uint32_t cf = cci[i] & 0xFFFFu;
    if ((uint32_t)i < n && (cf >> 5) == l) occw |= 1u << (cf & 31u);
  }
  bool moved = false;
#pragma unroll
  for (int i = 0; i < C::NAM; ++i) {
    if (!__any((uint32_t)i < n)) break;   // wave-uniform: no group has an agent i
    const uint32_t cf = cci[i] & 0xFFFFu, ct = cci[i] >> 16, kk = kki[i];
    const bool hit = ((ct >> 5) == l && ((occw >> (ct & 31u)) & 1u)) || (moved && (kk == kr || kk == kd1 || kk == kd2));
    const bool acc = (__ballot(hit) & gmask) == 0ull && (uint32_t)i < n;
    if (acc) {
      if ((cf >> 5) == l) occw &= ~(1u << (cf & 31u));
      if ((ct >> 5) == l) occw |= 1u << (ct & 31u);
      if (l == (uint32_t)i) moved = true;
    }
  }
  if (moved) s.ag = (s.ag & ~XY16) | utx | (uty << 16);
  // ---- expiry (core.py:303-306): requests whose expiry byte equals t close
  {
    const uint32_t eq = ~nz_hi(s.pe ^ ((s.t & 0xFFu) * 0x01010101u)) & SWAR_H;
    s.pt &= ~(((eq & nz_hi(s.pt)) >> 7) * 0xFFu);
  }
  // ---- pickups (core.py:309-335): every agent decides against the pre-pickup table, then the
  // points are cleared (two agents on one point both take its request)
  bool rew = false;
  {
    const uint32_t px = s.ag & 0xFFu, py = (s.ag >> 16) & 0xFFu;
    uint32_t cv = reinterpret_cast<const uint8_t*>(tbl)[cell_index((int)px, (int)py, D)];   // point + 1, 0 = none
    if (l >= n) cv = 0u;
    const uint32_t j = (cv - 1u) & 63u;
    const uint32_t tb = (grp_get(s.pt, j >> 2) >> (8u * (j & 3u))) & 0xFFu;
    const bool take = cv != 0u && ((s.ag >> 8) & 0xFFu) == 0xFFu && tb != 0u;
    const uint32_t dst = tbl[C::T.dst / 4 + (take ? tb - 1u : 0u)];   // x << 8 | y << 24 | 0x00FF00FF
    if (take) s.ag &= dst;
    rew = take;
    const uint64_t tk = row_or64(take ? 1ull << j : 0ull);
    s.pt &= ~expand_nib((uint32_t)(tk >> (4u * l)) & 0xFu);
  }
  s.am = wide_open_mask(s.pt, l);
  done = s.t >= T;                                                   // core.py:438
  // ---- regeneration (core.py:338-351): reopen k = R - P + |inactive| points
  {
    const uint64_t inactive = ~s.am & low_mask<C::P>();
    const uint32_t nin = (uint32_t)__popcll(inactive);
    nin_out = nin;
    // (a finished episode that is reset right away: its regeneration lands in state the reset replaces)
    const int kreq = (skip_regen_if_done && done) ? 0 : C::R - C::P + (int)nin;
    const uint32_t exp = (s.t + W) & 0xFFu;
    if (regen) {
      // injected: R positions into the ascending inactive list, then R targets; invalid draws are ignored
      for (int j = 0; j < C::R; ++j) {
        if (!__any(j < kreq)) break;
        const uint32_t rpos = (uint32_t)regen[j], tgi = (uint32_t)regen[C::R + j];
        const bool on = j < kreq && rpos < nin && tgi < (uint32_t)C::DP;
        const uint32_t sel = select_bit64(inactive, on ? rpos : 0u);
        wide_set_request<C>(s, l, on, sel, tgi, exp);
        if (on) s.am |= 1ull << sel;
      }
    } else if (__any(kreq > 0)) {
      // philox (REGEN stream, words 2j / 2j + 1 = item j's point / target; lane b holds block b)
      const uint4 blk = stream_block(k, gid, s.epi, s.t, PUR_REGEN, l);
      uint64_t left = inactive, used = 0;
      for (int j = 0; j < C::R; ++j) {
        if (!__any(j < kreq)) break;
        const uint32_t w1 = grp_get((j & 1) ? blk.z : blk.x, (uint32_t)(j >> 1));
        const uint32_t w2 = grp_get((j & 1) ? blk.w : blk.y, (uint32_t)(j >> 1));
        const bool on = j < kreq;
        const uint32_t sel = select_bit64(left, on ? __umulhi(w1, nin - (uint32_t)j) : 0u);
        const uint32_t tgi = select_bit64(~used & low_mask<C::DP>(), __umulhi(w2, (uint32_t)(C::DP - j)));
        if (on) {
          left &= ~(1ull << sel);
          used |= 1ull << tgi;
          s.am |= 1ull << sel;
        }
        wide_set_request<C>(s, l, on, sel, tgi, exp);
      }
    }
  }
  // ---- deliveries (core.py:354-368): the carried target cell equals the position (idle agents'
  // 0xFF target bytes never match; a pickup, interior, and a delivery, on the border, never share a step)
  if (l < n && ((s.ag >> 8) & XY16) == (s.ag & XY16)) {
    s.ag |= IDLE;
    rew = true;
  }
  s.fresh = 0u;
  return rew;
}

// The wide step kernel: `steps` iterations of {policy, step, optional auto-reset} with the state in
// registers, for wh_step_wide / wh_rollout_wide / wh_vector_step_wide.  Group g of the workgroup is
// env blockIdx.x * 16 + g.
template <class C, int POLICY>
__global__ __launch_bounds__(BT) void k_step_wide(StepParams a) {
  static_assert(C::NAM <= WL && C::PW <= WL, "one agent word and one pickup word per lane");
  __shared__ WideLds<C> L;
  load_tables<C>(L.tbl, a.tables);
  __syncthreads();
  const uint32_t* tbl = L.tbl;
  const int tid = threadIdx.x;
  const uint32_t l = (uint32_t)tid & (WL - 1);
  const int64_t e = (int64_t)blockIdx.x * WIDE_ENVS + (tid >> 4);
  const bool live = e < a.B && (!a.mask || a.mask[e]);   // group-uniform
  if (!__any(live)) return;                              // wave-uniform
  const int64_t es = e < a.B ? e : 0;                    // idle groups shadow env 0 and write nothing
  const uint64_t gmask = 0xFFFFull << ((uint32_t)tid & 48u);
  const int na = a.na;
  const int64_t B = a.B;
  const Keys k{a.k0, a.k1};
  const uint32_t gid = (uint32_t)(a.env_offset + es);
  // ---- load (host_engine.cpp load)
  WideEnv s;
  {
    const uint32_t hdr = a.state[es];
    s.t = hdr & 0xFFFFu;
    s.n = min((hdr >> 16) & 0xFFu, (uint32_t)na);
    s.fresh = (hdr >> 24) & 1u;
    s.epi = a.state[B + es];
    s.ag = l < s.n ? a.state[(int64_t)(2 + l) * B + es] : IDLE;
    const bool pl = l < (uint32_t)C::PW;
    s.pt = pl ? a.state[(int64_t)(2 + na + l) * B + es] : 0u;
    s.pe = pl ? a.state[(int64_t)(2 + na + C::PW + l) * B + es] : 0u;
    s.am = wide_open_mask(s.pt, l);
  }
  const bool stats = a.stats.episode_return != nullptr;
  uint32_t epr = stats ? a.stats.episode_return[es] : 0u;
  float ret = 0.0f;
  for (int stp = 0; stp < a.steps; ++stp) {
    uint32_t act = 4u;
    if (POLICY == POL_EXTERNAL) {
      if (l < (uint32_t)na) act = (uint32_t)a.actions[es * na + l];
    } else {
      act = wide_policy<C, POLICY>(s, tbl, k, gid, l, a.p);
    }
    bool done;
    uint32_t nin;
    const bool rew = wide_step<C>(s, tbl, k, gid, l, gmask, act, a.regen ? a.regen + es * 2 * C::R : nullptr,
                                  a.autoreset != 0, (uint32_t)a.T, (uint32_t)a.W, done, nin);
    const uint32_t rsum = (uint32_t)__popcll(__ballot(rew) & gmask);   // whole numbers: exact
    if (live) {
      if (a.rewards && l < (uint32_t)na) a.rewards[((int64_t)stp * B + e) * na + l] = rew ? 1.0f : 0.0f;
      if (l == 0u) {
        if (a.dones) a.dones[(int64_t)stp * B + e] = done ? 1 : 0;
        if (a.n_inactive) a.n_inactive[e] = (int32_t)nin;
      }
    }
    ret += (float)rsum;
    if (stats) {
      epr += rsum;
      if (__any(live && done)) flush_episodes(live && done && l == 0u, s.n, epr, a.stats);
      if (done) epr = 0u;
    }
    if (a.autoreset && __any(done)) {
      const WideEnv r = wide_reset<C>(s, tbl, k, gid, l, na, a.variable_n, (uint32_t)a.W);
      if (done) s = r;
    }
  }
  if (!live) return;
  // ---- store (host_engine.cpp store)
  if (l == 0u) {
    a.state[e] = s.t | (s.n << 16) | (s.fresh << 24);
    a.state[B + e] = s.epi;
    if (a.returns) a.returns[e] += ret;
    if (stats) a.stats.episode_return[e] = epr;
  }
  if (l < (uint32_t)na) a.state[(int64_t)(2 + l) * B + e] = l < s.n ? s.ag : IDLE;
  if (l < (uint32_t)C::PW) {
    a.state[(int64_t)(2 + na + l) * B + e] = s.pt;
    a.state[(int64_t)(2 + na + C::PW + l) * B + e] = s.pe;
  }
}
