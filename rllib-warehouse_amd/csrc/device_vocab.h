// device_vocab.h -- the device vocabulary of the lane-per-env kernels (device code; included by
// warehouse_amd.hip first, inside its anonymous namespace, after abi_args.h, philox.h and
// warehouse_amd.h).
//
// What every kernel header after it speaks in: the workgroup size and the build-time switches, the
// per-workgroup table layout (TableLayout, built on the host by build_tables()), a configuration's
// sizes (Cfg), the Philox stream helpers, the branch-free bit and SWAR helpers, an env's registers and
// LDS planes (Regs, Lds, Slots), and the table and env load / store.
constexpr int BT = 256;  // lanes (= envs) per workgroup
// Pickup-plane cell width: 16-bit cells put lanes 2k and 2k+1 in one LDS bank (b32-and-narrower
// accesses bank by dword mod 32 over 32-lane groups), a 2-way conflict on every access whose rows
// differ between the two lanes -- the move loop's target-byte lookups, the pickup clears and the
// regeneration stores.  32-bit cells (the upper half unused) give every lane of a group its own
// bank for twice the LDS, and measured slower anyway (Medium-8 +0.3 %, Large-16 +0.4 % per
// 200-step launch, profiles/r05_occ_ab.txt; round 4 the same), so the cells stay 16-bit.
using PkCell = uint16_t;
constexpr uint32_t PKW = sizeof(PkCell);
constexpr uint32_t ROWB = PKW * BT;   // bytes per pickup-point row of the LDS pickup plane

enum Policy { POL_EXTERNAL = 0, POL_GREEDY = 1, POL_RANDOM = 2 };
enum Purpose : uint32_t { PUR_RESET = 1, PUR_REGEN = 2, PUR_POLICY = 3, PUR_RANDOM = 4 };
constexpr int PH_ALL = 0, PH_PRE = 1, PH_REGEN = 2, PH_POLICY = 3;
#ifdef WH_ABLATION
constexpr bool kAblationBuild = true;    // ablation moves are arbitrary: keep the off-grid clamp
#else
constexpr bool kAblationBuild = false;
#endif

// -DWH_OBS_EB0=<n>: envs per workgroup of the observation kernel for the widest f32 rows (Large)
#ifndef WH_OBS_EB0
#define WH_OBS_EB0 4
#endif
constexpr int kObsEB[4] = {WH_OBS_EB0, 8, 16, 64};   // the observation kernel's instances
// The widest f32 rows (kObsEB[0]'s: Large) are written in chunks of WH_OBS_CHUNK float4s per workgroup
// (k_observe's CHUNK form; 0 = each workgroup writes its own envs' rows).  Large-16 sampler step
// 127 -> 109-112 us, wh_observe 110 -> 100-104 us (profiles/r06_obschunk_ab.txt, r06_obschunk2_ab.txt:
// 512 / 768 / 1280 / 1536 float4s, plain stores and 2 vs 4 float4s in flight compared).
#ifndef WH_OBS_CHUNK
#define WH_OBS_CHUNK 1024
#endif
constexpr int kObsChunk = WH_OBS_CHUNK;
#ifndef WH_FUSE_ROWS_MAX   // rows per env (bytes) up to which the sampler routes fuse step + rows (fuse_rows)
#define WH_FUSE_ROWS_MAX 4096
#endif
// Observation stores (same-box A/Bs, tools/obs_bench.py, sampler_probe.py and policy_probe.py;
// profiles/r05_l16rows_ab.txt, r05_ntm8_ab.txt, r05_ntsel_ab.txt): f32 rows nontemporal for rows of
// <= 1 KB or > 4 KB per env (Small / Large: observe -5 % / -2 %, Large-16's sampler route -3 %,
// Small-4's 1-step sampler -3 %), except in multi-step sampler fragments (Small-4 +11 %); plain for
// Medium's rows (nontemporal: observe +10 %, sampler step +24 %).  The fragment operand plain: stored
// nontemporal it is written 5-11 % faster but the policy network then reads it from HBM instead of
// the last-level cache, and the policy route is 1 % slower at Medium-8 (no gain at Large-16).
template <class C>
constexpr bool rows_nt() {
  return C::NAM * C::L * 4 <= 1024 || C::NAM * C::L * 4 > 4096;
}

// Agent counts up to which the move loop has the no-reverse-key variant (Large-16, whose step loop
// spills, measured 1 % slower with it).
constexpr int kRevSplitMaxNam = 9;
// Turns between the move loop's dependent pickup lookups (cell -> point row, point -> target byte,
// target -> delivery cell, then the decision): each lookup is issued kPickDist turns after the one
// it depends on, so its LDS latency is covered by that many turns of the serial chain.  Two turns:
// Medium-8 -1.0 %, Large-16 -1.0 % per 200-step launch against one (profiles/r05_pick_ab.txt); three
// turns +1.3 % / +0.9 % against two (profiles/r05_tune_ab.txt).
constexpr int kPickDist = 2;

constexpr uint32_t IDLE = 0xFF00FF00u;    // delivery-target bytes of an idle agent
constexpr uint32_t XY16 = 0x00FF00FFu;    // position bytes of an agent word

// Cell -> pickup table (u8 per cell).  Byte x | y << 8 (one v_perm of the packed position): its dword
// -- the LDS bank -- is x >> 2, so every lane of a wave reads one of D/4 banks (~8- to 13-way
// conflicts).  Skewed: byte 4x + 132y (one v_dot4_u32_u8 of the agent word), bank (x + y) mod 32.
// Same-box A/B (profiles/r05_step3_ab.txt): Large-16 -1.6 % per step (-2.9 % with the policy-block
// Philox hoist), Medium-8 +3 % -- so the skewed table is used from D = 20 (Large) on.
__host__ __device__ constexpr bool cell_skew(int D) { return D >= 20; }
__host__ __device__ constexpr int cell_bytes(int D) { return cell_skew(D) ? 132 * D : 256 * D; }
__host__ __device__ constexpr int cell_index(int x, int y, int D) { return cell_skew(D) ? 4 * x + 132 * y : (x | (y << 8)); }

// Shared (per-workgroup) table layout in bytes; built identically by build_tables() on the host.
struct TableLayout {
  int cell, rp, tag, dst, mv, valid, bytes;
  __host__ __device__ constexpr TableLayout(int D, int P, int DP, int NV)
      : cell(0), rp(cell_bytes(D)), tag(cell_bytes(D) + 4), dst(cell_bytes(D) + 8 * (P + 1)),   // rp/tag interleaved
        mv(cell_bytes(D) + 8 * (P + 1) + 4 * DP), valid(cell_bytes(D) + 8 * (P + 1) + 4 * DP + 48),
        bytes(cell_bytes(D) + 8 * (P + 1) + 4 * DP + 48 + 4 * NV) {}
};

template <int D_, int R_, int NR_, int NAM_>
struct Cfg {
  static constexpr int D = D_, R = R_, NR = NR_, NAM = NAM_;
  static constexpr int P = 4 * NR * NR;
  static constexpr int DP = 4 * (D - 4);
  static constexpr int PW = P / 4;
  static constexpr int NV = (D - 2) * (D - 2) - P;      // interior cells that are not pickups
  static constexpr TableLayout T = TableLayout(D, P, DP, NV);
  static constexpr int TBLW = T.bytes / 4;
  static constexpr int TBL4 = (TBLW + 3) / 4;           // 16-byte chunks (device copy padded to them)
  static constexpr int L = 9 * R + 1;                    // observation row length
  static_assert(D <= 32, "positions are 5-bit fields (occupancy rows are 32-bit words)");
  static_assert(P <= 64 && DP <= 64, "bitmask sets hold at most 64 points");
  static_assert(NAM <= R, "agents <= requests (core.py:89)");
};

typedef short short2v __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ short2v as_s2(uint32_t v) { return __builtin_bit_cast(short2v, v); }
__device__ __forceinline__ uint32_t as_u(short2v v) { return __builtin_bit_cast(uint32_t, v); }

// ----------------------------------------------------------------------------- small helpers
__device__ __forceinline__ uint32_t comp(const uint4& v, int i) {
  return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w));
}

struct Keys {
  uint32_t k0, k1;
};

// Block b of stream (env, episode, t, purpose).
__device__ __forceinline__ uint4 stream_block(const Keys& k, uint32_t env, uint32_t ep, uint32_t t,
                                              uint32_t purpose, uint32_t b) {
  return philox10(make_uint4(env, ep, t, (purpose << 24) | b), k.k0, k.k1);
}

// Sequential reader for streams whose word indices are only known at run time (reset).
struct Reader {
  Keys k;
  uint32_t env, ep, t, purpose;
  int cur;
  uint4 blk;
  __device__ Reader(Keys k_, uint32_t env_, uint32_t ep_, uint32_t t_, uint32_t p_)
      : k(k_), env(env_), ep(ep_), t(t_), purpose(p_), cur(-1), blk(make_uint4(0, 0, 0, 0)) {}
  __device__ __forceinline__ uint32_t word(int j) {
    const int b = j >> 2;
    if (b != cur) {
      blk = stream_block(k, env, ep, t, purpose, (uint32_t)b);
      cur = b;
    }
    return comp(blk, j & 3);
  }
};

// Branch-free selects without VCC: a one-wave-per-SIMD kernel pays for every v_cmp -> SGPR mask ->
// v_cndmask round trip (measured: tools/oprate3.hip), while v_bitop3 is a plain full-rate VALU op.
// Masks are 0 / 0xFFFFFFFF in VGPRs; every consumer goes through the bitop3 builtin so LLVM cannot
// fold the mask arithmetic back into compare + select.
constexpr uint32_t TA = 0xF0, TB = 0xCC, TC = 0xAA;   // truth-table columns of operands 0, 1, 2
template <uint32_t TT>
__device__ __forceinline__ uint32_t bop3(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, (unsigned char)(TT & 0xFFu));
}
// Sign bit -> 0 / all-ones.  As inline asm: LLVM turns ashr(a - b, 31) into a carry-out compare
// plus v_cndmask (the round trip this file avoids).
__device__ __forceinline__ uint32_t sgn(uint32_t x) {
  uint32_t r;
  asm("v_ashrrev_i32 %0, 31, %1" : "=v"(r) : "v"(x));
  return r;
}
// The same sign mask as v_bfe_i32 x, 31, 1 through the builtin: no inline asm, so the hazard
// recognizer does not pad the next VALU with an s_nop (select_bit64 chains five of them per call);
// where LLVM would rewrite it into a compare (a difference of two values) the asm form stays.
__device__ __forceinline__ uint32_t sgn_bfe(uint32_t x) { return (uint32_t)__builtin_amdgcn_sbfe((int)x, 31u, 1u); }
__device__ __forceinline__ uint32_t mask_z(uint32_t x) { return sgn(x - 1u); }   // x == 0 (x < 2^31)
__device__ __forceinline__ uint32_t msel(uint32_t m, uint32_t a, uint32_t b) { return bop3<(TA & TB) | (~TA & TC)>(m, a, b); }

// Index of the r-th (0-based) set bit of m (r < popcount(m)).  Binary search over popcounts with
// the rank kept as sr = -1 - r: popcount(x) + sr is negative exactly when r >= popcount(x), and is
// then the rank left for the upper part.  Selects are v_bitop3 on sign masks (no VCC).
__device__ __forceinline__ uint32_t select_bit64(uint64_t m, uint32_t r) {
  uint32_t sr = ~r;
  uint32_t u = (uint32_t)__popc((uint32_t)m) + sr;
  uint32_t g = sgn_bfe(u);
  uint32_t w = msel(g, (uint32_t)(m >> 32), (uint32_t)m);
  sr = msel(g, u, sr);
  const uint32_t half = bop3<TA & TB>(g, 32u, 0u);
  // binary search inside w: the field of width k at offset base (v_bfe) instead of shifting w
  uint32_t base = 0;
#pragma unroll
  for (int k = 16; k >= 1; k >>= 1) {
    u = (uint32_t)__popc(__builtin_amdgcn_ubfe(w, base, (uint32_t)k)) + sr;
    g = sgn_bfe(u);
    if (k > 1) sr = msel(g, u, sr);
    base = bop3<(TA & TB) | TC>(g, (uint32_t)k, base);
  }
  return base | half;
}

// high bit of every nonzero byte
__device__ __forceinline__ uint32_t nz_hi(uint32_t x) {
  return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}
// 4 byte-flags (bit 7 of each byte) -> 4-bit nibble
__device__ __forceinline__ uint32_t nib_of(uint32_t hi) { return ((hi >> 7) * 0x00204081u) >> 21 & 0xFu; }
// 4-bit nibble -> 0xFF byte mask (full-rate 24-bit multiply)
__device__ __forceinline__ uint32_t expand_nib(uint32_t nib) {
  const uint32_t ones = __umul24(nib, 0x00204081u) & 0x01010101u;
  return (ones << 8) - ones;
}

// packed i16 max/min, pinned: hipcc rewrites clamp(x, -1, 1) on i16 pairs into per-half
// compare/select cascades (it recognises sign(x)); one v_pk_* op per bound is what we want.
__device__ __forceinline__ uint32_t pk_max_i16(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_pk_max_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ uint32_t pk_min_i16(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_pk_min_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ uint32_t pk_sub_i16(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_pk_sub_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// clamp(p + d) per 16-bit lane: the reference keeps the old coordinate when a +-1 move leaves
// [0, D) (core.py:284-287), which for unit moves is exactly a clamp to [0, D-1].
template <int D>
__device__ __forceinline__ uint32_t step16(uint32_t p, uint32_t d) {
  short2v v = as_s2(p) + as_s2(d);
  v = __builtin_elementwise_max(v, (short2v){0, 0});
  v = __builtin_elementwise_min(v, (short2v){(short)(D - 1), (short)(D - 1)});
  return as_u(v);
}

// action index of a unit step packed as (dx, dy) i16 pair: MOVES[a] = (a//3-1, a%3-1), core.py:38
__device__ __forceinline__ uint32_t action_of(uint32_t d) {
  const short2v v = as_s2(d);
  return (uint32_t)(3 * ((int)v.x + 1) + ((int)v.y + 1));
}
// an action outside 0 .. 8 is "stay"
__device__ __forceinline__ uint32_t valid_action(uint32_t action) { return action > 8u ? 4u : action; }

// Rare wave-uniform branches of the step loop (expiry pass, grid rebuild, resets, random moves): marked
// cold so that block placement keeps their code out of the hot path's instruction stream.
#define WH_RARE(x) __builtin_expect(!!(x), 0)

// Phase labels in the device assembly for instruction-count analysis (`make asm` defines
// WH_PHASE_MARKS).  Not in the library: each label is an asm volatile with a memory clobber, a
// scheduling barrier for memory operations -- without them Large-16 runs 0.9 % and Medium-8 0.3 %
// faster per 200-step launch (profiles/r06_nomarks_ab.txt).
#ifdef WH_PHASE_MARKS
#define WH_PHASE_MARK(name) asm volatile("; PHASE " #name ::: "memory")
#else
#define WH_PHASE_MARK(name) ((void)0)
#endif

// A byte read from LDS as the 32-bit value the load instruction leaves (ds_read_u8 zero-extends).
// Opaque to LLVM: knowing the value's 8 bits it narrows the mins and the merges of the two move loops
// that consume it to 8 / 16 bits and widens the results again, a v_and per lookup in the step loop.
__device__ __forceinline__ uint32_t lds_byte(const uint8_t* p) {
  uint32_t v = *p;
  asm("" : "+v"(v));
  return v;
}

template <class C>
struct Regs {
  uint32_t hdr, epi;
  uint32_t ag[C::NAM];
  uint64_t am;   // open requests (bit j = pickup point j has one; kept in registers across steps)
  // Wave-uniform first step of the expiry phase: W, since a request opened at t0 >= 0 lives W
  // steps, or 0 if some lane was loaded holding one that expires sooner (no episode reaches that).
  uint32_t wskip;
};

template <class C>
struct Lds {
  alignas(16) uint32_t tbl[4 * C::TBL4];
  uint32_t occ[C::D][BT];        // occupancy row y: bit x
  // Pickup point j of lane tid: low byte = request target + 1 (0 = none), high byte = expiry step
  // (low 8 bits).  Row P is scratch: predicated stores of lanes with nothing to write go there.
  // One cell per (point, lane) makes every per-point access a single ds op whose address is
  // j * BT + tid, and keeps the pickup table out of the VGPRs.
  PkCell pkp[C::P + 1][BT];
  // Agent words when processing in action-dict order; afterwards the reward-row staging area.
  // Wave w only ever touches its own 64 columns [64w, 64w + 64) of every row.
  alignas(16) uint32_t agl[C::NAM][BT];
  // Cell (x | y << 16) -> pickup index + 1, 0 for other cells: one v_perm (the byte index
  // x | y << 8) + one ds_read_u8; the point's row in pkp is then one v_lshl_add away (row_byte).
  __device__ __forceinline__ uint32_t cell_row(uint32_t xy16) const {
    if constexpr (cell_skew(C::D)) {
      // one v_dot4_u32_u8 of the agent word's bytes [x, dx, y, dy] with [4, 0, 132, 0]
      const uint32_t i = __builtin_amdgcn_udot4(xy16, 0x00840004u, 0u, false);
      return lds_byte(reinterpret_cast<const uint8_t*>(tbl) + i);
    } else {
      return lds_byte(reinterpret_cast<const uint8_t*>(tbl) + __builtin_amdgcn_perm(xy16, xy16, 0x0C0C0200u));
    }
  }

  // (pickup cell, greedy tag) of point j: one 8-byte LDS read
  __device__ __forceinline__ uint2 rtag(uint32_t j) const {
    return reinterpret_cast<const uint2*>(&tbl[C::T.rp / 4])[j];
  }
  __device__ __forceinline__ uint32_t mv(uint32_t a) const { return tbl[C::T.mv / 4 + a]; }
  __device__ __forceinline__ uint32_t valid_cell(uint32_t v) const { return tbl[C::T.valid / 4 + v]; }
  __device__ __forceinline__ uint32_t target_byte(uint32_t j, int tid) const {
    return *reinterpret_cast<const uint8_t*>(&pkp[j][tid]);
  }
  __device__ __forceinline__ void clear_target(uint32_t j, int tid) {
    *reinterpret_cast<uint8_t*>(&pkp[j][tid]) = 0;
  }
  // Target byte of the point whose cell_row() value is cv (0: the row before pkp -- garbage,
  // never used).
  __device__ __forceinline__ uint32_t pkp_offset() const {
    return (uint32_t)(reinterpret_cast<const char*>(&pkp[0][0]) - reinterpret_cast<const char*>(this));
  }
  __device__ __forceinline__ const uint8_t* row_byte(uint32_t cv, int tid) const {
    return reinterpret_cast<const uint8_t*>(this) + (pkp_offset() - ROWB) + cv * ROWB + PKW * tid;
  }
  __device__ __forceinline__ uint8_t* row_byte(uint32_t cv, int tid) {
    return reinterpret_cast<uint8_t*>(this) + (pkp_offset() - ROWB) + cv * ROWB + PKW * tid;
  }
  __device__ __forceinline__ uint32_t row_target(uint32_t cv, int tid) const { return lds_byte(row_byte(cv, tid)); }
  // Delivery cell of a target byte (target + 1; 0 reads the word before the table: never used) in
  // agent-word form: x << 8 | y << 24 in the target bytes, ones in the position bytes, so a pickup
  // is one AND of the (idle: 0xFF target bytes) agent word.
  __device__ __forceinline__ uint32_t dst_tb(uint32_t tb) const { return tbl[C::T.dst / 4 - 1 + tb]; }
};

// Reset slots (fused rollout only: their own __shared__ object in that k_step instance, so the
// other step instances and k_reset do not carry them): lane tid's NEXT episode's reset state,
// precomputed for the whole wave at once (reset_philox<..., TO_SLOT>) and consumed when the lane ends
// its episode (reset_from_slot): agent words, R requests (point | (target + 1) << 8), open mask,
// header, and the episode the slot was computed for (valid iff rs_ep == epi + 1).
template <class C>
struct Slots {
  uint32_t rs_ag[C::NAM][BT];
  uint16_t rs_req[C::R][BT];
  uint32_t rs_am[2][BT], rs_hdr[BT], rs_ep[BT];
};
struct NoSlots {};

// Every 16-byte load of a lane is issued before its first LDS write, so the prologue pays one
// memory round trip.  (A strided `for` loop over words compiled to load -> vmcnt(0) -> ds_write per
// iteration: ~10 serial round trips per launch at Medium-8, most of a short launch's fixed cost.)
// Split in two: issue_tables() puts the loads in flight first (the table is L2-resident: it comes back
// well before the state planes from HBM), commit_tables() writes them to LDS -- the waitcnt pass then
// waits for the table loads only (vmcnt counts in order), with the state loads still in flight.
// Chunk i (16 bytes per lane) of the table, as plain values: a struct or array of them crossing
// the state loads was kept in memory by LLVM (promoted to LDS, 32 bytes per lane, or put in scratch).
template <class C>
constexpr int kTableChunks = (C::TBL4 + BT - 1) / BT;
template <class C>
__device__ __forceinline__ bool table_lane(int i) {
  return i < kTableChunks<C> && (C::TBL4 % BT == 0 || i + 1 < kTableChunks<C> || (int)threadIdx.x + i * BT < C::TBL4);
}
template <class C>
__device__ __forceinline__ uint4 issue_table_chunk(const uint32_t* __restrict__ tables, int i) {
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (table_lane<C>(i)) v = reinterpret_cast<const uint4*>(tables)[threadIdx.x + i * BT];
  return v;
}
template <class C>
__device__ __forceinline__ void commit_table_chunk(uint32_t* dst, int i, uint4 v) {
  if (table_lane<C>(i)) reinterpret_cast<uint4*>(dst)[threadIdx.x + i * BT] = v;
}
template <class C>
__device__ __forceinline__ void load_tables(uint32_t* dst, const uint32_t* __restrict__ tables) {
  static_assert(kTableChunks<C> <= 2, "tables of at most 2 x 4 KB");
  const uint4 v0 = issue_table_chunk<C>(tables, 0), v1 = issue_table_chunk<C>(tables, 1);
  commit_table_chunk<C>(dst, 0, v0);
  commit_table_chunk<C>(dst, 1, v1);
}

template <class C>
__device__ __forceinline__ uint64_t active_mask(const uint32_t (&pt)[C::PW]) {
  uint64_t am = 0;
#pragma unroll
  for (int w = 0; w < C::PW; ++w) am |= (uint64_t)nib_of(nz_hi(pt[w])) << (4 * w);
  return am;
}

template <int N>
__device__ __forceinline__ uint64_t low_mask() {
  return N >= 64 ? ~0ull : ((1ull << N) - 1ull);
}

// The packed words of one env, loaded to registers.  Word plane w of the workgroup's envs is
// st + w * B + e0 (e0 = the workgroup's first env): a wave-uniform pointer, advanced by B with two
// scalar adds per plane, and the lane's offset tid * 4 -- global loads in SGPR-base form, so no
// per-lane 64-bit address arithmetic (it was ~100 VALU, a third of them v_mad_u64_u32, in front of
// the first load).  Issue order = use order: the header and the pickup planes (target, expiry
// pairs: the pickup plane is built from them while the rest arrive), then the episode counter and
// the agent words (first used in the step loop).
template <class C>
struct RawEnv {
  uint32_t hdr, epi, ag[C::NAM], pt[C::PW], pm[C::PW];
};

template <class C>
__device__ __forceinline__ void load_env_issue(RawEnv<C>& r, const uint32_t* __restrict__ st, int64_t B,
                                               int64_t e0, int tid, int na) {
  const uint32_t* pl = st + e0;
  r.hdr = pl[tid];
  const uint32_t* pt = pl + (int64_t)(2 + na) * B;
  const uint32_t* pm = pt + (int64_t)C::PW * B;
#pragma unroll
  for (int w = 0; w < C::PW; ++w) {
    r.pt[w] = pt[tid];
    r.pm[w] = pm[tid];
    pt += B;
    pm += B;
  }
  pl += B;
  r.epi = pl[tid];
#pragma unroll
  for (int i = 0; i < C::NAM; ++i) {
    pl += B;
    r.ag[i] = (i < na) ? pl[tid] : IDLE;
  }
}

// SWAR byte ops on 4 packed unsigned bytes (H = the bytes' high bits)
constexpr uint32_t SWAR_H = 0x80808080u;
__device__ __forceinline__ uint32_t swar_sub(uint32_t x, uint32_t y) {   // (x_b - y_b) mod 256 per byte
  return ((x | SWAR_H) - (y & ~SWAR_H)) ^ ((x ^ ~y) & SWAR_H);
}
__device__ __forceinline__ uint32_t swar_lt(uint32_t x, uint32_t y) {    // bit 7 of byte b: x_b < y_b
  return (((~x & y) | (~(x ^ y) & swar_sub(x, y))) & SWAR_H);
}

template <class C>
__device__ __forceinline__ void load_env_finish(Regs<C>& s, Lds<C>& L, const RawEnv<C>& r, uint32_t W, int tid) {
  s.hdr = r.hdr;
  s.epi = r.epi;
#pragma unroll
  for (int i = 0; i < C::NAM; ++i) s.ag[i] = r.ag[i];
  // pickup cell j = target byte | expiry byte << 8: two cells per v_perm, stored as 16-bit halves
#pragma unroll
  for (int w = 0; w < C::PW; ++w) {
    const uint32_t lo = __builtin_amdgcn_perm(r.pm[w], r.pt[w], 0x05010400u);   // cells 4w, 4w+1
    const uint32_t hi = __builtin_amdgcn_perm(r.pm[w], r.pt[w], 0x07030602u);   // cells 4w+2, 4w+3
    L.pkp[4 * w][tid] = (uint16_t)lo;
    L.pkp[4 * w + 1][tid] = (uint16_t)(lo >> 16);
    L.pkp[4 * w + 2][tid] = (uint16_t)hi;
    L.pkp[4 * w + 3][tid] = (uint16_t)(hi >> 16);
  }
  s.am = active_mask<C>(r.pt);
  // An open request expires at step t0 + ((expiry byte - t0) mod 256), as the expiry phase counts;
  // it is "early" if that is before W, i.e. its steps left < W - t0 (never when t0 >= W).  Four
  // points per SWAR test.
  const uint32_t t0 = s.hdr & 0xFFFFu;
  const uint32_t thr = t0 < W ? W - t0 : 0u;          // <= 255
  uint32_t early = 0;
#pragma unroll
  for (int w = 0; w < C::PW; ++w)
    early |= nz_hi(r.pt[w]) & swar_lt(swar_sub(r.pm[w], (t0 & 0xFFu) * 0x01010101u), thr * 0x01010101u);
  // (LLVM folds this select of two uniform values into every step's expiry test, `any early || t >= W`,
  // five instructions there.  Pinned in a scalar register through v_readfirstlane it left one compare
  // in the step and measured slower -- Medium-8 +0.8 %, Large-16 +5 % per 200-step launch,
  // profiles/fused_constants_ab.txt -- so it is not.)
  s.wskip = __any(early != 0u) ? 0u : W;
}

template <class C>
__device__ __forceinline__ void store_env(const Regs<C>& s, const Lds<C>& L, uint32_t* __restrict__ st,
                                          int64_t B, int64_t e0, int na, int tid) {
  uint32_t* pl = st + e0;   // word planes as in load_env_issue: wave-uniform base + lane offset
  pl[tid] = s.hdr;
  pl += B;
  pl[tid] = s.epi;
#pragma unroll
  for (int i = 0; i < C::NAM; ++i)
    if (i < na) {
      pl += B;
      pl[tid] = s.ag[i];
    }
  uint32_t* pt = pl + B;
  uint32_t* pm = pt + (int64_t)C::PW * B;
#pragma unroll
  for (int w = 0; w < C::PW; ++w) {
    // four 16-bit cells -> target bytes and expiry bytes: two shift-ors and two v_perm
    const uint32_t lo = (uint32_t)L.pkp[4 * w][tid] | ((uint32_t)L.pkp[4 * w + 1][tid] << 16);
    const uint32_t hi = (uint32_t)L.pkp[4 * w + 2][tid] | ((uint32_t)L.pkp[4 * w + 3][tid] << 16);
    pt[tid] = __builtin_amdgcn_perm(hi, lo, 0x06040200u);
    pm[tid] = __builtin_amdgcn_perm(hi, lo, 0x07050301u);
    pt += B;
    pm += B;
  }
}
