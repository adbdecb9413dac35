// reset.h -- the four reset forms of the lane-per-env kernels (device code; included by
// warehouse_amd.hip after device_vocab.h): reset_philox (every lane its own env; to registers or to the
// reset slots, one lane or a whole wave), reset_from_slot and reset_lane (one env by the whole wave),
// reset_injected (parity mode).
// ----------------------------------------------------------------------------- reset
// core.py:167-221 (philox draws): spawn on interior non-pickup cells, open R requests.
// Law (the same as the reference's np.random.choice(P, R) paired with choice(Dp, R)): a uniform
// R-subset of the pickup points, each given a distinct uniformly random delivery target.  The
// subset comes from Floyd's algorithm (item j: r = uniform over [0, m] with m = P - R + j, take r
// unless already taken, else m), one test and two ors per item; the targets are a uniform ordered
// R-tuple without replacement (the r-th unused delivery point, r uniform over Dp - j), so pairing
// them with the points in Floyd's order is a uniform injection.  NAC >= 0 is the agent count at
// compile time (the fused rollout): every stream word then has a fixed place in the precomputed
// Philox blocks, and the whole reset is straight-line code.
// TO_SLOT: the same draws and results for every lane, written to the lane's reset slot (Lds::rs_*)
// instead of its registers and pickup plane, for episode epi + 1.
// The pickup-plane rows (and, with occ, the occupancy rows) of the wave's 64 columns cleared with
// 16-byte stores, for a reset of every lane of a full wave (synchronised episodes end together): 5
// stores instead of 36 (Medium) per lane, 4 instead of 16 for the grid.
template <class C>
__device__ __forceinline__ void clear_wave_columns(Lds<C>& L, int tid, bool occ) {
  const int wb = tid & ~63, lane = tid & 63;
  constexpr int CPL = 16 / PKW, LPR = 64 / CPL, RPS = 64 / LPR;   // cells per lane, lanes per row, rows
#pragma unroll
  for (int j0 = 0; j0 < C::P; j0 += RPS) {
    const int j = j0 + lane / LPR;
    if (C::P % RPS == 0 || j < C::P)
      *reinterpret_cast<uint4*>(&L.pkp[j][wb + CPL * (lane % LPR)]) = make_uint4(0u, 0u, 0u, 0u);
  }
  if (occ) {
#pragma unroll
    for (int y0 = 0; y0 < C::D; y0 += 4) {
      const int y = y0 + (lane >> 4);
      if (C::D % 4 == 0 || y < C::D)
        *reinterpret_cast<uint4*>(&L.occ[y][wb + 4 * (lane & 15)]) = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

// WAVE: every lane of a full wave resets (the caller checked): the pickup plane is cleared
// wave-wide with clear_wave_columns.
template <class C, int NAC = -1, bool TO_SLOT = false, bool WAVE = false>
__device__ __forceinline__ void reset_philox(Regs<C>& s, Lds<C>& L, const Keys& k, uint32_t gid,
                                             int na_rt, int variable_n, uint32_t W, int tid,
                                             Slots<C>* RS = nullptr) {
  WH_PHASE_MARK(reset);
  const uint32_t ep = s.epi + 1u;
  const int na = NAC >= 0 ? NAC : na_rt;
  constexpr int NB = NAC >= 0 ? (1 + NAC + 2 * C::R + 3) / 4 : 1;
  uint4 blk[NB];
  if constexpr (NAC >= 0) {
#pragma unroll
    for (int b = 0; b < NB; ++b) blk[b] = stream_block(k, gid, ep, 0u, PUR_RESET, (uint32_t)b);
  }
  Reader rd(k, gid, ep, 0u, PUR_RESET);
  auto word = [&](int j) -> uint32_t {
    if constexpr (NAC >= 0) return comp(blk[j >> 2], j & 3);
    else return rd.word(j);
  };
  const uint32_t n = variable_n ? 1u + __umulhi(word(0), (uint32_t)na) : (uint32_t)na;
#pragma unroll
  for (int i = 0; i < C::NAM; ++i) {
    uint32_t a = IDLE;
    if (i < na) {
      const uint32_t v = __umulhi(word(1 + i), (uint32_t)C::NV);
      const uint32_t cell = L.valid_cell(v);
      a = (i < (int)n) ? (cell | IDLE) : IDLE;
    }
    if (TO_SLOT) RS->rs_ag[i][tid] = a;
    else s.ag[i] = a;
  }
  if (!TO_SLOT) {
    if constexpr (WAVE) {
      clear_wave_columns<C>(L, tid, true);
    } else {
#pragma unroll
      for (int j = 0; j < C::P; ++j) L.pkp[j][tid] = 0;
    }
  }
  const uint32_t wexp = (W & 0xFFu) << 8;   // opened at t = 0: expires at step W
  uint32_t plo = 0, phi = 0;                // Floyd's subset so far
  uint32_t sel[C::R], tg[C::R];
#pragma unroll
  for (int j = 0; j < C::R; ++j) {
    constexpr int M0 = C::P - C::R;
    const uint32_t m = (uint32_t)(M0 + j);
    const uint32_t r = __umulhi(word(1 + na + 2 * j), m + 1u);
    sel[j] = r;
    if (j > 0) {   // taken already: bit r of the subset, moved to bit 63 by one 64-bit shift
      const uint64_t sh = (((uint64_t)phi << 32) | plo) << (63u - r);
      sel[j] = msel(sgn((uint32_t)(sh >> 32)), m, r);
    }
    const uint64_t sb = 1ull << sel[j];
    plo |= (uint32_t)sb;
    phi |= (uint32_t)(sb >> 32);
    tg[j] = __umulhi(word(2 + na + 2 * j), (uint32_t)(C::DP - j));   // rank among unused targets
  }
  // ranks -> targets (item j: the tg[j]-th delivery point not taken by items < j), decoded from
  // the last item back: every later item at or above item j's value moves up one.  The same
  // values as a rank selection per item, as independent compare-adds instead of a serial chain.
#pragma unroll
  for (int j = C::R - 2; j >= 0; --j)
#pragma unroll
    for (int i = j + 1; i < C::R; ++i) tg[i] += 1u - ((tg[i] - tg[j]) >> 31);   // + (tg[i] >= tg[j])
  if (TO_SLOT) {
#pragma unroll
    for (int j = 0; j < C::R; ++j) RS->rs_req[j][tid] = (uint16_t)(sel[j] | ((tg[j] + 1u) << 8));
    RS->rs_am[0][tid] = plo;
    RS->rs_am[1][tid] = phi;
    RS->rs_hdr[tid] = (n << 16) | (1u << 24);
    RS->rs_ep[tid] = ep;
  } else {
#pragma unroll
    for (int j = 0; j < C::R; ++j) L.pkp[sel[j]][tid] = (uint16_t)((tg[j] + 1u) | wexp);
    s.am = ((uint64_t)phi << 32) | plo;
    s.hdr = (n << 16) | (1u << 24);
    s.epi = ep;
  }
  WH_PHASE_MARK(reset_end);
}

// The reset of the env of lane l of this wave from its reset slot (valid: rs_ep == epi + 1), by
// the whole wave: agent words and request cells read across lanes (lane i reads field i of lane
// l's column), the pickup-plane and occupancy columns cleared and written one cell per lane.
// Bit-identical to reset_philox<C, NA> (plus the occupancy clear) for that env, for ~40 issue slots
// instead of a Philox block per lane, a Floyd chain on wave-uniform values and the rank decode.
template <class C, int NA>
__device__ __forceinline__ void reset_from_slot(Regs<C>& s, Lds<C>& L, const Slots<C>& RS, uint32_t W, int tid, int l) {
  WH_PHASE_MARK(slot_reset);
  const int lane = tid & 63;
  const int col = (tid & ~63) + l;
  const uint32_t me = mask_z((uint32_t)(lane ^ l));
  const uint32_t av = RS.rs_ag[lane < NA ? lane : 0][col];
  const uint32_t rq = RS.rs_req[lane < C::R ? lane : 0][col];
  const uint32_t alo = RS.rs_am[0][col], ahi = RS.rs_am[1][col], hdr = RS.rs_hdr[col];
#pragma unroll
  for (int i = 0; i < C::NAM; ++i)
    s.ag[i] = msel(me, i < NA ? (uint32_t)__builtin_amdgcn_readlane(av, i) : IDLE, s.ag[i]);
  if (lane < C::P) L.pkp[lane][col] = 0;
  if (lane < C::D) L.occ[lane][col] = 0u;
  if (lane < C::R) L.pkp[rq & 0xFFu][col] = (uint16_t)((rq >> 8) | ((W & 0xFFu) << 8));   // after the clear
  s.am = ((uint64_t)msel(me, ahi, (uint32_t)(s.am >> 32)) << 32) | msel(me, alo, (uint32_t)s.am);
  s.hdr = msel(me, hdr, s.hdr);
  s.epi = msel(me, s.epi + 1u, s.epi);
}

// The same philox reset for ONE env -- the env of lane l of this wave -- computed by the whole
// wave: a Philox block per lane (lane b holds block b), words read across lanes, the subset and
// target arithmetic on wave-uniform values (target ranks by v_mbcnt + ballot), and lane l's LDS
// column (pickup cells, occupancy rows) written one cell per lane.  Bit-identical to
// reset_philox<C, NA> (plus the occupancy clear) for that env, at a fraction of its issue cost:
// the fused rollout uses it when a single lane of the wave ends its episode, which is what
// desynchronised episodes produce (env ends are spread over the steps, B/T per step).
template <class C, int NA>
__device__ __forceinline__ void reset_lane(Regs<C>& s, Lds<C>& L, const Keys& k, uint32_t gid,
                                           int variable_n, uint32_t W, int tid, int l) {
  WH_PHASE_MARK(lane_reset);
  const int lane = tid & 63;
  const int col = (tid & ~63) + l;                      // lane l's LDS column
  const uint32_t me = mask_z((uint32_t)(lane ^ l));      // all-ones on lane l
  const uint32_t gid_l = __builtin_amdgcn_readlane(gid, l);
  const uint32_t ep = __builtin_amdgcn_readlane(s.epi, l) + 1u;
  constexpr int NB = (1 + NA + 2 * C::R + 3) / 4;
  static_assert(NB <= 64, "one Philox block per lane");
  const uint4 mine = stream_block(k, gid_l, ep, 0u, PUR_RESET, (uint32_t)(lane < NB ? lane : 0));
  auto word = [&](int j) -> uint32_t { return __builtin_amdgcn_readlane(comp(mine, j & 3), j >> 2); };
  const uint32_t n = variable_n ? 1u + __umulhi(word(0), (uint32_t)NA) : (uint32_t)NA;
  // every spawn cell is read (all reads in flight together) and slots >= n are then masked: with
  // `i < n` as the condition of the read, n being wave-uniform, each read sat in its own scalar
  // branch behind a waitcnt -- NA serial LDS round trips per reset
  uint32_t cell[C::NAM];
#pragma unroll
  for (int i = 0; i < C::NAM; ++i)
    cell[i] = i < NA ? L.valid_cell(__umulhi(word(1 + i), (uint32_t)C::NV)) : 0u;
#pragma unroll
  for (int i = 0; i < C::NAM; ++i) {
    const uint32_t live = sgn((uint32_t)i - n);   // all-ones: i < n
    s.ag[i] = msel(me, bop3<(TA & TB) | TC>(live, cell[i], IDLE), s.ag[i]);
  }
  if (lane < C::P) L.pkp[lane][col] = 0;
  if (lane < C::D) L.occ[lane][col] = 0u;
  const uint32_t wexp = (W & 0xFFu) << 8;
  // points: Floyd's subset on wave-uniform values (a short scalar chain); lane j < R keeps item j
  uint64_t S = 0;
  uint32_t selv = (uint32_t)C::P, tgv = 0;
#pragma unroll
  for (int j = 0; j < C::R; ++j) {
    const uint32_t m = (uint32_t)(C::P - C::R + j);
    const uint32_t r = __umulhi(word(1 + NA + 2 * j), m + 1u);
    const uint32_t sel = (j > 0 && ((S >> r) & 1ull)) ? m : r;
    S |= 1ull << sel;
    // (computed on every lane, then selected: as `lane == j ? rank : tgv` each item was an
    // exec-masked branch, ~8 issue slots of branching per item)
    const uint32_t rank = __umulhi(word(2 + NA + 2 * j), (uint32_t)(C::DP - j));   // r2_j
    const uint32_t mj = mask_z((uint32_t)(lane ^ j));
    selv = msel(mj, sel, selv);
    tgv = msel(mj, rank, tgv);
  }
  // targets: item j is the r2_j-th delivery point not taken by items < j.  Decoded in parallel
  // (lane j holds item j): from the last item back, every later item at or above item j's value
  // moves up one -- the same values as the per-lane rank selection, without its serial chain.
#pragma unroll
  for (int j = C::R - 2; j >= 0; --j) {
    const uint32_t xj = __builtin_amdgcn_readlane(tgv, j);
    tgv += (lane > j && lane < C::R && tgv >= xj) ? 1u : 0u;
  }
  const uint32_t valv = (tgv + 1u) | wexp;
  if (lane < C::R) L.pkp[selv][col] = (uint16_t)valv;     // after the clear (LDS ops in order)
  s.am = ((uint64_t)msel(me, (uint32_t)(S >> 32), (uint32_t)(s.am >> 32)) << 32) | msel(me, (uint32_t)S, (uint32_t)s.am);
  s.hdr = msel(me, (n << 16) | (1u << 24), s.hdr);
  s.epi = msel(me, ep, s.epi);
}

template <class C>
__device__ __forceinline__ void reset_injected(Regs<C>& s, Lds<C>& L, int64_t e, int na,
                                               const int32_t* spawn, const int32_t* pickups,
                                               const int32_t* targets, const int32_t* nn,
                                               uint32_t W, int tid) {
  const uint32_t n = nn ? min((uint32_t)nn[e], (uint32_t)na) : (uint32_t)na;
#pragma unroll
  for (int i = 0; i < C::NAM; ++i) {
    uint32_t a = IDLE;
    if (i < na && i < (int)n) {
      const uint32_t x = min((uint32_t)spawn[(e * na + i) * 2], (uint32_t)(C::D - 1));
      const uint32_t y = min((uint32_t)spawn[(e * na + i) * 2 + 1], (uint32_t)(C::D - 1));
      a = x | (y << 16) | IDLE;
    }
    s.ag[i] = a;
  }
#pragma unroll
  for (int j = 0; j < C::P; ++j) L.pkp[j][tid] = 0;
  const uint32_t wexp = (W & 0xFFu) << 8;   // opened at t = 0: expires at step W
  uint64_t opened = 0;
  for (int j = 0; j < C::R; ++j) {
    const uint32_t sel = (uint32_t)pickups[e * C::R + j];
    const uint32_t tg = (uint32_t)targets[e * C::R + j];
    if (sel >= (uint32_t)C::P || tg >= (uint32_t)C::DP) continue;   // invalid injected draw: ignored
    opened |= 1ull << sel;
    L.pkp[sel][tid] = (uint16_t)((tg + 1u) | wexp);
  }
  s.am = opened;
  s.hdr = (n << 16) | (1u << 24);
  s.epi = s.epi + 1u;
}
