// warehouse_amd.hip -- gfx950 kernels + C ABI for the batched warehouse hot path.
//
// Design (DESIGN.md has the rationale and the measurements behind each choice):
//  * ONE LANE PER ENV.  The per-env work of core.py:262-442 is a short, mostly serial integer
//    program (sequential collision resolution, core.py:279-300).  One env per lane with the batch
//    across lanes makes every HBM access a coalesced word plane (state[w * B + e]) and shares each
//    issued instruction among 64 envs.  With B = 65,536 that is one wave per SIMD, so the kernel
//    is VALU-issue bound and every instruction per env-step counts.
//  * 16-bit coordinate pairs.  An agent word is x | dx<<8 | y<<16 | dy<<24 (dx,dy = delivery
//    target cell, 0xFF = idle): a move is 3 packed-i16 ops (the reference's "keep the old
//    coordinate off the grid" rule equals a clamp for +-1 moves, core.py:282-287), a delivery test
//    is one compare (core.py:354-362) and Manhattan distance is one v_sad_hi_u8, which also
//    carries the pickup index and cell as a 16-bit tag so a v_min gives argmin-first-wins
//    (solvers.py:53-58).
//  * SWAR on packed bytes.  Pickup tables are 1 byte per point, 4 per register: expiry
//    (core.py:303-306) and clearing/opening (core.py:330-351) run 4 points per VALU op; the set of
//    open requests is a 64-bit mask kept in registers across fused steps.
//  * Per-lane LDS scratch for the data-dependent lookups (occupancy rows core.py:275-291, pickup
//    target bytes core.py:327-329), laid out [word][lane] so every lane hits its own bank, and no
//    data-dependent branches: LDS side effects are predicated through neutral operands.
//  * Counter-based Philox streams (no RNG state in HBM) or injected draws (parity mode).
// The kernels live in the headers included below, one per concern.  This file keeps the host side
// (from "host side" down): the device tables, the kernel registry and the launch decisions, and the
// C ABI.  Two things are shared with the host engine (host_engine.cpp): where the warehouse's points
// and cells are (geometry.h), and which arguments a call is refused for (abi_args.h), which every
// entry point that takes a config goes through.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <mutex>
#include <type_traits>
#include <unordered_set>
#include <new>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "abi_args.h"
#include "geometry.h"
#include "philox.h"
#include "sac_formula.h"
#include "warehouse_amd.h"

namespace {

// The device side, one header per concern, in dependency order (each header's first lines say what
// it needs before it); all of them are part of this translation unit's anonymous namespace.
#include "device_vocab.h"   // constants, Cfg / TableLayout, bit helpers, Regs / Lds / Slots, table and env load / store
#include "reset.h"          // reset_philox, reset_from_slot, reset_lane, reset_injected
#include "policy.h"         // policy_walk, policy_steps
#include "step_env.h"       // step_env, obs_src, store_rewards, check_env (assert mode)
#include "step_params.h"    // StepParams, flush_episodes
// The 16-lanes-per-env form of the step (k_step_wide): wh_step_wide / wh_rollout_wide / wh_vector_step_wide.
#include "step_wide.h"
#include "step_loops.h"     // run_steps, FastRun, run_steps_fast, k_step, k_reset, the WH_TIMING stamps
#include "observe.h"        // ObsSrc, stream_rows / stream_frags, the image build, k_observe
#include "replay.h"         // k_replay_put, k_replay_gather
#include "step_record.h"    // RecordParams, k_step_record: the recorded step (wh_replay_record)
#include "prio.h"           // k_prio_fill, k_prio_update, k_prio_sample
#include "sac.h"            // k_sac_td (the row arithmetic: sac_formula.h, shared with the host engine)
#include "sac_loss.h"       // k_sac_loss, k_sac_loss_finish (after sac.h: its span constants)
#include "adam.h"           // k_adam
#include "sampler.h"        // FImg, SampLds, write_image, k_sampler
#include "pack.h"           // k_pack, k_unpack

// ----------------------------------------------------------------------------- host side
int hip_err(hipError_t e) { return e == hipSuccess ? WH_OK : WH_EHIP + (int)e; }

// Which calls are refused, and a step-family call reduced to one struct, are the ABI's own rules
// (abi_args.h, shared with the host engine); what follows is what this back end adds: the device
// tables, the kernel instances, and which of them a call launches.
using Geometry = wh_abi::Shape;
using wh_abi::StepCall;
static_assert(wh_abi::POLICY_EXTERNAL == POL_EXTERNAL && WH_POLICY_GREEDY == POL_GREEDY && WH_POLICY_RANDOM == POL_RANDOM &&
              wh_abi::PHASE_POLICY == PH_POLICY && WH_PHASE_ALL == PH_ALL, "StepCall carries the kernels' codes");

// Host copy of the per-workgroup tables, same layout as TableLayout; where the points and cells are
// is geometry.h's business (core.py:170-199), how they are packed into words is written here:
//   cell  [256*D] u8 : (x | y << 8) -> pickup index + 1, 0 = not a pickup cell
//   rp/tag [P+1] u32 pairs, interleaved (the policy reads both with one 8-byte LDS read):
//          rp  = pickup cell as x | y << 16; [P] = far-away cell (never nearest)
//          tag = pickup << 10 | x << 5 | y   (greedy argmin tag, solvers.py:53-58);
//                [P] = the null cell (D/2, D/2): where fresh-reset agents head (core.py:233-236)
//   dst   [Dp]   u32 : delivery cell in agent-word target bytes, x << 8 | y << 24 | 0x00FF00FF
//   mv    [12]   u32 : MOVES[a] as packed i16 (dx, dy) (core.py:38)
//   valid [NV]   u32 : interior non-pickup cells x | y << 16, ascending (x, y) (spawn, core.py:191-199)
std::vector<uint32_t> build_tables(const Geometry& g, int* bad) {
  const int D = g.D;
  *bad = 0;
  if (D > 32 || wh_geo::racks_overlap(g.racks, g.NR)) { *bad = 1; return {}; }
  std::vector<uint8_t> cell(cell_bytes(D), 0);
  std::vector<uint32_t> rp(g.P + 1), tag(g.P + 1);
  rp[g.P] = 0x00FF00FFu;
  tag[g.P] = (63u << 10) | ((uint32_t)(D / 2) << 5) | (uint32_t)(D / 2);   // pickup << 10 | y << 5 | x
  for (int j = 0; j < g.P; ++j) {
    const wh_geo::Cell c = wh_geo::pickup_cell(g.racks, g.NR, j);
    cell[cell_index(c.x, c.y, D)] = (uint8_t)(j + 1);
    rp[j] = (uint32_t)c.x | ((uint32_t)c.y << 16);
    tag[j] = ((uint32_t)j << 10) | ((uint32_t)c.y << 5) | (uint32_t)c.x;
  }
  std::vector<uint32_t> dst(g.DP);
  for (int d = 0; d < g.DP; ++d) {
    const wh_geo::Cell c = wh_geo::delivery_cell(d, D);
    dst[d] = ((uint32_t)c.x << 8) | ((uint32_t)c.y << 24) | XY16;
  }
  std::vector<uint32_t> mv(12, 0);
  for (int a = 0; a < 9; ++a) {
    const int dx = a / 3 - 1, dy = a % 3 - 1;
    mv[a] = (uint32_t)(uint16_t)(int16_t)dx | ((uint32_t)(uint16_t)(int16_t)dy << 16);
  }
  std::vector<uint32_t> valid;
  wh_geo::spawn_cells(g.racks, g.NR, D, [&valid](int x, int y) { valid.push_back((uint32_t)x | ((uint32_t)y << 16)); });
  std::vector<uint32_t> words(cell.size() / 4, 0);
  memcpy(words.data(), cell.data(), cell.size());
  for (int j = 0; j <= g.P; ++j) {
    words.push_back(rp[j]);
    words.push_back(tag[j]);
  }
  words.insert(words.end(), dst.begin(), dst.end());
  words.insert(words.end(), mv.begin(), mv.end());
  words.insert(words.end(), valid.begin(), valid.end());
  return words;
}

struct TableEntry {
  int device, D, NR, words;
  int racks[WH_MAX_RACKS];
  uint32_t* dev;
};
std::mutex g_tab_mu;
std::vector<TableEntry> g_tabs;

// Device copy of the tables for (device, geometry); allocated once per geometry and device.  The
// device is the launch stream's (not the calling thread's current device), so a kernel never reads
// tables that live on another GPU.
int device_tables(const Geometry& g, int expect_words, hipStream_t stream, const uint32_t** out) {
  int dev = 0;
  hipError_t he = stream ? hipStreamGetDevice(stream, &dev) : hipGetDevice(&dev);
  if (he != hipSuccess) return hip_err(he);
  std::lock_guard<std::mutex> lk(g_tab_mu);
  for (auto& t : g_tabs)
    if (t.device == dev && t.D == g.D && t.NR == g.NR && !memcmp(t.racks, g.racks, sizeof(int) * g.NR)) {
      *out = t.dev;
      return t.words == expect_words ? WH_OK : WH_ENOTSUP;
    }
  int bad = 0;
  std::vector<uint32_t> w = build_tables(g, &bad);
  if (bad || (int)w.size() != expect_words) return WH_ENOTSUP;
  int cur = 0;
  he = hipGetDevice(&cur);
  if (he != hipSuccess) return hip_err(he);
  if (cur != dev && (he = hipSetDevice(dev)) != hipSuccess) return hip_err(he);
  uint32_t* d = nullptr;
  const size_t padded = (w.size() + 3) / 4 * 16;   // load_tables reads whole 16-byte chunks
  he = hipMalloc(&d, padded);
  if (he == hipSuccess) he = hipMemset(d, 0, padded);
  if (he == hipSuccess) he = hipMemcpy(d, w.data(), w.size() * 4, hipMemcpyHostToDevice);
  if (cur != dev) (void)hipSetDevice(cur);
  if (he != hipSuccess) return hip_err(he);
  TableEntry t{dev, g.D, g.NR, (int)w.size(), {0}, d};
  memcpy(t.racks, g.racks, sizeof(int) * g.NR);
  g_tabs.push_back(t);
  *out = d;
  return WH_OK;
}

// ---- kernel registry: (D, R, NR, NAM) instances
struct Kernels {
  int D, R, NR, NAM;
  void (*step[3])(StepParams);
  void (*step_fast[3])(StepParams);   // [policy]: greedy / random fused rollouts (NAM even), else null
  void (*step_fast_eps0)(StepParams);   // the greedy one for launches with p = 0: no random-move code
  void (*step_ordered)(StepParams);
  void (*step_wide[3])(StepParams);   // [policy]: 16 lanes per env (k_step_wide)
  void (*sampler[3])(StepParams, float*);   // [policy]: fused step + rows (k_sampler), NAM even, else null
  void (*sampler_multi[3])(StepParams, float*);   // [policy]: the same, K steps per launch (greedy / random)
  void (*vsampler[2])(StepParams, float*);  // [ordered]: wh_vector_step's step + rows (external actions)
  void (*reset)(ResetParams);
  void (*observe[4])(const uint32_t*, int64_t, int, const uint32_t*, float*, int, uint4*);   // kObsEB[i] envs per WG
  void (*observe_chunk)(const uint32_t*, int64_t, int, const uint32_t*, float*, int, uint4*);   // kObsChunk float4s per WG
  void (*replay_put)(PutParams);
  void (*step_record[3])(RecordParams);   // [policy]: the recorded step (k_step_record)
  void (*replay_gather[4])(GatherParams);   // kObsEB[i] samples per WG (the instances the gather uses: 0, 2, 3)
  int tblw, nv;
};

// Large (R = 16) dispatches no k_sampler: with 16 agent slots its rows (9.3 KB per env) pass the fuse
// limit, and with 2-8 slots the step code spills at two waves per SIMD (220-544 B of scratch,
// tools/kernel_resources.py), which fused_ok() refuses.  Those instances are not built (unless an A/B
// build raises the limit), so no kernel with a private segment is left in the dict-order route.
template <class C>
constexpr bool kSamplerBuilt = C::R < 16 || WH_FUSE_ROWS_MAX > 4096;

template <int D, int R, int NR, int NAM>
Kernels make_kernels() {
  using C = Cfg<D, R, NR, NAM>;
  Kernels k;
  k.D = D; k.R = R; k.NR = NR; k.NAM = NAM;
  k.step[0] = k_step<C, POL_EXTERNAL, false, false>;
  k.step[1] = k_step<C, POL_GREEDY, false, false>;
  k.step[2] = k_step<C, POL_RANDOM, false, false>;
  k.step_fast[0] = nullptr;   // (set below for even agent counts: wh_vector_step's common case)
  k.step_fast_eps0 = nullptr;
  k.sampler[0] = k.sampler[1] = k.sampler[2] = nullptr;
  k.sampler_multi[0] = k.sampler_multi[1] = k.sampler_multi[2] = nullptr;
  // the multi-step sampler holds the step's LDS, its reset slots and two image buffers
  constexpr bool sampler_fits = sizeof(Lds<C>) + sizeof(Slots<C>) + sizeof(SampLds<C, 2>) <= 160 * 1024;
  if constexpr (NAM % 2 == 0) {
    k.step_fast[0] = k_step<C, POL_EXTERNAL, false, true>;
    k.step_fast[1] = k_step<C, POL_GREEDY, false, true>;
    k.step_fast[2] = k_step<C, POL_RANDOM, false, true>;
    k.step_fast_eps0 = k_step<C, POL_GREEDY, false, true, false>;
    if constexpr (kSamplerBuilt<C>) {
      k.sampler[0] = k_sampler<C, POL_EXTERNAL, false, true>;
      k.sampler[1] = k_sampler<C, POL_GREEDY, false, true>;
      k.sampler[2] = k_sampler<C, POL_RANDOM, false, true>;
    }
    if constexpr (sampler_fits && kSamplerBuilt<C>) {
      k.sampler_multi[1] = k_sampler<C, POL_GREEDY, false, true, true>;
      k.sampler_multi[2] = k_sampler<C, POL_RANDOM, false, true, true>;
    }
  } else {
    k.step_fast[1] = k.step_fast[2] = nullptr;
  }
  // the dict-order step holds the step's LDS and the entries' move keys; a shape too large for a
  // workgroup's 160 KB fails here instead of at its first launch
  static_assert(sizeof(Lds<C>) + sizeof(OKeys<C>) <= 160 * 1024, "k_step<..., ORDERED> exceeds the LDS of a workgroup");
  k.step_ordered = k_step<C, POL_EXTERNAL, true, false>;
  k.step_wide[0] = k_step_wide<C, POL_EXTERNAL>;
  k.step_wide[1] = k_step_wide<C, POL_GREEDY>;
  k.step_wide[2] = k_step_wide<C, POL_RANDOM>;
  k.vsampler[0] = k.vsampler[1] = nullptr;
  if constexpr (kSamplerBuilt<C>) {
    k.vsampler[0] = k_sampler<C, POL_EXTERNAL, false, false>;
    // the dict-order instance also holds the entries' move keys (OKeys: 4 * NAM x 512 bytes)
    if constexpr (sizeof(Lds<C>) + sizeof(SampLds<C, 1>) + sizeof(OKeys<C>) <= 160 * 1024)
      k.vsampler[1] = k_sampler<C, POL_EXTERNAL, true, false>;
  }
  k.reset = k_reset<C>;
  k.observe[0] = k_observe<C, kObsEB[0]>;
  k.observe[1] = k_observe<C, kObsEB[1]>;
  k.observe[2] = k_observe<C, kObsEB[2]>;
  k.observe[3] = k_observe<C, kObsEB[3]>;
  k.observe_chunk = kObsChunk > 0 ? k_observe<C, kObsEB[0], kObsChunk> : nullptr;
  k.replay_put = k_replay_put<C>;
  k.step_record[0] = k_step_record<C, POL_EXTERNAL>;
  k.step_record[1] = k_step_record<C, POL_GREEDY>;
  k.step_record[2] = k_step_record<C, POL_RANDOM>;
  k.replay_gather[0] = k_replay_gather<C, kObsEB[0]>;
  k.replay_gather[1] = nullptr;
  k.replay_gather[2] = k_replay_gather<C, kObsEB[2]>;
  k.replay_gather[3] = k_replay_gather<C, kObsEB[3]>;
  k.tblw = C::TBLW;
  k.nv = C::NV;
  return k;
}

const std::vector<Kernels>& registry() {
#ifdef WH_ONLY_MEDIUM8   // analysis builds (tools/lds_stalls.py): one instance, fast to compile
  static const std::vector<Kernels> r = {make_kernels<16, 9, 3, 8>()};
#elif defined(WH_ONLY_LARGE16)
  static const std::vector<Kernels> r = {make_kernels<20, 16, 4, 16>()};
#elif defined(WH_ONLY_SMALL4)
  static const std::vector<Kernels> r = {make_kernels<12, 4, 2, 4>()};
#else
  static const std::vector<Kernels> r = {
      // WarehouseSmall  (variants.py:19-32): D=12, R=4, racks [4, 8]
      make_kernels<12, 4, 2, 2>(), make_kernels<12, 4, 2, 4>(),
      // WarehouseMedium (variants.py:35-47): D=16, R=9, racks [4, 8, 12]
      make_kernels<16, 9, 3, 2>(), make_kernels<16, 9, 3, 4>(), make_kernels<16, 9, 3, 8>(),
      make_kernels<16, 9, 3, 9>(),
      // WarehouseLarge  (variants.py:50-62): D=20, R=16, racks [4, 8, 12, 16]
      make_kernels<20, 16, 4, 2>(), make_kernels<20, 16, 4, 4>(), make_kernels<20, 16, 4, 8>(),
      make_kernels<20, 16, 4, 16>(),
  };
#endif
  return r;
}

// A fused step + rows kernel (k_sampler) runs two waves per SIMD, so its step code gets 256
// registers instead of 512: configurations whose step needs more spill to scratch there (Large-16)
// and keep the two launches.  Decided once per kernel from its private segment size.
bool fused_ok(void (*kern)(StepParams, float*)) {
  static std::mutex mu;
  static std::vector<std::pair<const void*, bool>> seen;
  std::lock_guard<std::mutex> lk(mu);
  for (const auto& p : seen)
    if (p.first == reinterpret_cast<const void*>(kern)) return p.second;
  hipFuncAttributes at;
  const bool ok = hipFuncGetAttributes(&at, reinterpret_cast<const void*>(kern)) == hipSuccess && at.localSizeBytes == 0;
  seen.emplace_back(reinterpret_cast<const void*>(kern), ok);
  return ok;
}

// The fused step + rows launch pays while an env's rows are small: at Large-16 (9.3 KB of rows per
// env, one 512-lane workgroup per CU by LDS) it streams the rows slower than k_observe's small
// workgroups -- 165 vs 127 us per sampler step for the two launches (profiles/r06_l16fuse_ab.txt,
// with the fused instance free of scratch); Small-4 13.2 vs 15.1, Medium-8 34.7 vs 40.3
// (profiles/r05_step3_ab.txt).  So configurations with more than WH_FUSE_ROWS_MAX bytes of rows per
// env take the two launches.
bool fuse_rows(const Geometry& g) { return 4 * g.NA * g.L <= WH_FUSE_ROWS_MAX; }

const Kernels* pick(const Geometry& g) {
  const Kernels* best = nullptr;
  for (const auto& k : registry())
    if (k.D == g.D && k.R == g.R && k.NR == g.NR && k.NAM >= g.NA && (!best || k.NAM < best->NAM))
      best = &k;
  return best;
}

// The kernel instance of a valid geometry and, for a batch that launches, its device tables.
int locate(const Geometry& g, int64_t B, void* stream, const Kernels** kk, const uint32_t** tab) {
  *kk = pick(g);
  if (!*kk) return WH_ENOTSUP;
  *tab = nullptr;
  if (B == 0) return WH_OK;   // an empty batch launches nothing: no device, no tables
  return device_tables(g, (*kk)->tblw, (hipStream_t)stream, tab);
}

inline dim3 grid_for(int64_t B) { return dim3((unsigned)((B + BT - 1) / BT)); }
inline dim3 grid_wide(int64_t B) { return dim3((unsigned)((B + WIDE_ENVS - 1) / WIDE_ENVS)); }   // k_step_wide: 16 envs per workgroup

}  // namespace

// =============================================================================== C ABI
extern "C" {

#ifdef WH_TIMING
int wh_debug_times(uint64_t* out, int32_t n) {   // timing builds only (not in the header)
  if (!out || n < 0 || n > kTimeWaves * kTimeSlots) return WH_EINVAL;
  hipError_t he = hipDeviceSynchronize();
  if (he == hipSuccess) he = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wh_times), (size_t)n * 8, 0, hipMemcpyDeviceToHost);
  return he == hipSuccess ? WH_OK : hip_err(he);
}
#endif

int wh_check_read(uint64_t* out, int32_t clear) {
#ifdef WH_CHECK
  if (!out) return WH_EINVAL;
  unsigned long long v[4];
  hipError_t he = hipDeviceSynchronize();
  if (he == hipSuccess) he = hipMemcpyFromSymbol(v, HIP_SYMBOL(g_wh_check), sizeof(v), 0, hipMemcpyDeviceToHost);
  if (he != hipSuccess) return hip_err(he);
  for (int i = 0; i < 4; ++i) out[i] = v[i];
  if (clear) {
    const unsigned long long z[4] = {0, 0, 0, 0};
    he = hipMemcpyToSymbol(HIP_SYMBOL(g_wh_check), z, sizeof(z), 0, hipMemcpyHostToDevice);
    if (he != hipSuccess) return hip_err(he);
  }
  return WH_OK;
#elif defined(WH_COUNT_REV)
  if (!out) return WH_EINVAL;
  unsigned long long v[2];
  hipError_t he = hipDeviceSynchronize();
  if (he == hipSuccess) he = hipMemcpyFromSymbol(v, HIP_SYMBOL(g_wh_revcount), sizeof(v), 0, hipMemcpyDeviceToHost);
  if (he != hipSuccess) return hip_err(he);
  out[0] = v[0];
  out[1] = v[1];
  out[2] = out[3] = 0;
  if (clear) {
    const unsigned long long z[2] = {0, 0};
    he = hipMemcpyToSymbol(HIP_SYMBOL(g_wh_revcount), z, sizeof(z), 0, hipMemcpyHostToDevice);
    if (he != hipSuccess) return hip_err(he);
  }
  return WH_OK;
#else
  (void)out;
  (void)clear;
  return WH_ENOTSUP;
#endif
}

int wh_query(const wh_config* cfg, wh_layout* out) {
  Geometry g;
  int rc = wh_abi::check_config(cfg, &g);
  if (rc) return rc;
  const Kernels* k = pick(g);
  if (!k) return WH_ENOTSUP;
  if (out) {
    out->words_per_env = g.words;
    out->num_pickups = g.P;
    out->num_deliveries = g.DP;
    out->obs_len = g.L;
    out->kernel_agents = k->NAM;
  }
  return WH_OK;
}

int wh_pack(const wh_config* cfg, int64_t B, const int32_t* pos, const int32_t* agent_target,
            const int32_t* pickup_target, const int32_t* pickup_timer, const int32_t* t,
            const int32_t* n, const uint8_t* fresh, const uint32_t* episode, uint32_t* state,
            void* stream) {
  Geometry g;
  const int rc = wh_abi::pack_call(&g, cfg, B, state, pos, agent_target, pickup_target, pickup_timer, t, n, fresh, episode);
  if (rc || B == 0) return rc;
  PackParams a{state, nullptr, B, g.NA, g.P, g.P / 4, g.D, const_cast<int32_t*>(pos),
               const_cast<int32_t*>(agent_target), const_cast<int32_t*>(pickup_target),
               const_cast<int32_t*>(pickup_timer), const_cast<int32_t*>(t), const_cast<int32_t*>(n),
               const_cast<uint8_t*>(fresh), const_cast<uint32_t*>(episode)};
  hipLaunchKernelGGL(k_pack, grid_for(B), dim3(BT), 0, (hipStream_t)stream, a);
  return hip_err(hipGetLastError());
}

int wh_unpack(const wh_config* cfg, int64_t B, const uint32_t* state, int32_t* pos,
              int32_t* agent_target, int32_t* pickup_target, int32_t* pickup_timer, int32_t* t,
              int32_t* n, uint8_t* fresh, uint32_t* episode, void* stream) {
  Geometry g;
  const int rc = wh_abi::pack_call(&g, cfg, B, state, pos, agent_target, pickup_target, pickup_timer, t, n, fresh, episode);
  if (rc || B == 0) return rc;
  PackParams a{nullptr, state, B, g.NA, g.P, g.P / 4, g.D, pos, agent_target, pickup_target,
               pickup_timer, t, n, fresh, episode};
  hipLaunchKernelGGL(k_unpack, grid_for(B), dim3(BT), 0, (hipStream_t)stream, a);
  return hip_err(hipGetLastError());
}

int wh_reset(const wh_config* cfg, int64_t B, uint32_t* state, const uint8_t* mask,
             const wh_reset_draws* draws, int32_t variable_n, uint64_t seed, int64_t env_offset,
             void* stream) {
  Geometry g;
  const Kernels* k;
  const uint32_t* tab;
  int rc = wh_abi::reset_call(&g, cfg, B, state, draws);
  if (rc || (rc = locate(g, B, stream, &k, &tab)) || B == 0) return rc;
  ResetParams a{state, B, g.NA, g.W, tab, mask,
                draws ? draws->spawn : nullptr, draws ? draws->pickups : nullptr,
                draws ? draws->targets : nullptr, draws ? draws->n : nullptr,
                draws ? 1 : 0, variable_n ? 1 : 0,
                wh_abi::lo32(seed), wh_abi::hi32(seed), env_offset};
  hipLaunchKernelGGL(k->reset, grid_for(B), dim3(BT), 0, (hipStream_t)stream, a);
  return hip_err(hipGetLastError());
}

}  // extern "C"

// A step launch with every argument resolved: what launch_step enqueues, and what a prepared
// launch (wh_rollout_prepare / wh_launch_run) replays without re-validating anything.  It keeps the
// geometry and the kernel instance it was resolved for: the entries that write rows go on from them
// to a fused step + rows kernel or to k_observe.
struct wh_launch {
  void (*kern)(StepParams);
  dim3 grid;
  hipStream_t stream;
  StepParams a;
  Geometry g;
  const Kernels* k;
};

// Live handles of wh_rollout_prepare: run / free of anything else (a freed or foreign pointer) is
// refused with WH_EINVAL instead of being dereferenced.
static std::mutex g_launch_mu;
static std::unordered_set<const wh_launch*> g_launches;
static bool launch_live(const wh_launch* l) {
  std::lock_guard<std::mutex> lk(g_launch_mu);
  return g_launches.count(l) != 0;
}

// The kernel argument of a checked call (abi_args.h): the one place a StepParams is filled.
static StepParams step_params(const StepCall& c, const uint32_t* tables) {
  StepParams a{};
  a.state = c.state;
  a.B = c.B;
  a.na = c.g.NA;
  a.T = c.g.T;
  a.W = c.g.W;
  a.tables = tables;
  a.actions = c.actions;
  a.order = c.order;   // non-NULL: the action-dict order path (k_step<..., ORDERED>)
  a.ol = c.ol;
  a.rewards = c.rewards;
  a.dones = c.dones;
  a.returns = c.returns;
  a.regen = c.regen;
  a.n_inactive = c.n_inactive;
  a.actions_out = c.actions_out;
  a.p = c.p;
  a.k0 = wh_abi::lo32(c.seed);
  a.k1 = wh_abi::hi32(c.seed);
  a.env_offset = c.env_offset;
  a.steps = c.steps;
  a.phase = c.phase;
  a.autoreset = c.autoreset;
  a.variable_n = c.variable_n;
#ifdef WH_ABLATION
  const char* abl = getenv("WH_ABLATE");   // timing experiments only (tools/ablate.py)
  a.ablate = abl ? atoi(abl) : 0;
#endif
  if (c.stats) a.stats = *c.stats;
  a.mask = c.mask;
  a.state_out = c.state_out;   // (wh_sampler_step_to: every env is live, each lane stores its whole state)
  return a;
}

// The back end's part of a checked call: the kernel instance, the device tables, the step kernel.
static int resolve_step(const StepCall& c, void* stream, wh_launch* out) {
  const uint32_t* tab;
  const int rc = locate(c.g, c.B, stream, &out->k, &tab);
  if (rc) return rc;
  const Kernels* k = out->k;
  const int policy = c.policy;
  const StepParams a = step_params(c, tab);
  void (*kern)(StepParams) = (a.order != nullptr && policy == POL_EXTERNAL) ? k->step_ordered : k->step[policy];
  // the fused rollout's common case (run_steps_fast); rows of 16 (NAM % 4 == 0) or 8 bytes
  const uintptr_t ralign = (k->NAM % 4 == 0) ? 15u : 7u;
  if (k->step_fast[policy] && a.phase == PH_ALL && a.rewards && a.dones && !a.returns &&
      !a.stats.episode_return && !a.mask && !a.order && !a.regen && !a.n_inactive && a.autoreset &&
      c.g.NA == k->NAM && ((uintptr_t)a.rewards & ralign) == 0)
    kern = (policy == POL_GREEDY && !(a.p > 0.0f)) ? k->step_fast_eps0 : k->step_fast[policy];   // (the kernel's own test of p)
  const bool wide = c.lanes == WH_WIDE_LANES;   // k_step_wide (csrc/step_wide.h): 16 lanes per env
  out->kern = wide ? k->step_wide[policy] : kern;
  out->grid = wide ? grid_wide(c.B) : grid_for(c.B);
  out->stream = (hipStream_t)stream;
  out->a = a;
  out->g = c.g;
  return WH_OK;
}

// Did the step resolve to the fused rollout's fast instance of `policy` (either greedy form)?  The
// k_sampler instances run the same step, so the sampler routes fuse the rows exactly then.
static bool fast_step(const wh_launch& l, int policy) {
  return l.kern == l.k->step_fast[policy] || (policy == POL_GREEDY && l.k->step_fast_eps0 && l.kern == l.k->step_fast_eps0);
}

static int enqueue(const wh_launch& l) {
  if (l.a.B == 0) return WH_OK;
  hipLaunchKernelGGL(l.kern, l.grid, dim3(BT), 0, l.stream, l.a);
  return hip_err(hipGetLastError());
}

static int launch_step(const StepCall& c, void* stream) {
  wh_launch l;
  const int rc = resolve_step(c, stream, &l);
  return rc ? rc : enqueue(l);
}

// Envs per workgroup of the observation rows of a geometry, as an index into kObsEB: `rows` f32 rows
// are written, `frags` the fragment-order operand (either or both).  k_observe launches the instance
// (observe_launch); the replay gather, which always writes as if for f32 rows, its own of the same size.
static int obs_group_sel(const Geometry& g, bool rows, bool frags) {
  // envs per workgroup (same-box A/Bs, tools/obs_bench.py and tools/sampler_probe.py): f32 rows 64
  // for Small-4's 592 B/env rows, 16 for Medium-8's 2.6 KB, 4 for Large-16's 9.3 KB
  // (profiles/r05_obseb0_ab.txt: 8 -> 4 is 119.5 -> 115.2 us, and 133 -> 130 us for the sampler
  // route, profiles/r05_obseb1_ab.txt 120.6 -> 114.8 us); the fragment operand alone 64 / 16 / 8
  // (Large-16: 16 is 3 % and 4 is 20 % slower than 8, profiles/r05_obseb1_ab.txt / r05_obseb0_ab.txt)
  const int row_bytes = 4 * g.NA * g.L;
  int sel = row_bytes <= 1024 ? 3 : (row_bytes <= 4096 ? 2 : (rows ? 0 : 1));
  // the fragment operand is written in whole 32-row tiles per workgroup: groups of 64 envs hold
  // 64 * NA rows, a multiple of 32 for every agent count (e.g. Medium with 9 agents, whose f32-row
  // grouping of 16 envs = 144 rows does not)
  if (frags && (kObsEB[sel] * g.NA) % 32 != 0) sel = 3;
  return sel;
}

// k_observe for B > 0 envs of a resolved geometry: f32 rows to `obs`, the policy network's
// fragment-order operand to `xfrag` (16-byte aligned), or both.
static int observe_launch(const Geometry& g, const Kernels* k, const uint32_t* tab, int64_t B, const uint32_t* state,
                          float* obs, void* xfrag, void* stream) {
  const int quads = ((g.NA * g.L) % 4 == 0) && ((uintptr_t)obs % 16 == 0);
  const int sel = obs_group_sel(g, obs != nullptr, xfrag != nullptr);
  const int ebx = kObsEB[sel];
  const int64_t qe = (int64_t)g.NA * g.L / 4;
  if (sel == 0 && !xfrag && quads && k->observe_chunk && kObsChunk <= (ebx - 1) * qe + 1) {
    hipLaunchKernelGGL(k->observe_chunk, dim3((unsigned)((B * qe + kObsChunk - 1) / kObsChunk)), dim3(BT), 0,
                       (hipStream_t)stream, state, B, g.NA, tab, obs, quads, static_cast<uint4*>(xfrag));
    return hip_err(hipGetLastError());
  }
  hipLaunchKernelGGL(k->observe[sel], dim3((unsigned)((B + ebx - 1) / ebx)), dim3(BT), 0,
                     (hipStream_t)stream, state, B, g.NA, tab, obs, quads, static_cast<uint4*>(xfrag));
  return hip_err(hipGetLastError());
}

static int observe_impl(const wh_config* cfg, int64_t B, const uint32_t* state, float* obs, void* xfrag,
                        void* stream) {
  Geometry g;
  const Kernels* k;
  const uint32_t* tab;
  int rc = wh_abi::observe_call(&g, cfg, B, state, obs, xfrag);
  if (rc || (rc = locate(g, B, stream, &k, &tab)) || B == 0) return rc;
  return observe_launch(g, k, tab, B, state, obs, xfrag, stream);
}

// May the rows of a resolved step be written by its own launch (a k_sampler instance `fk`: the step
// on half of each workgroup, every env's rows by all of it)?  Only while an env's rows are small
// (fuse_rows) and whole float4s, and `fk` keeps its registers (fused_ok); WH_SAMPLER_UNFUSED=1 forces
// the two launches (A/B runs).
static bool rows_fusable(const wh_launch& l, void (*fk)(StepParams, float*), const float* obs) {
  static const bool unfused = getenv("WH_SAMPLER_UNFUSED") != nullptr;
  return obs && !unfused && fuse_rows(l.g) && fk && fused_ok(fk) && (l.g.NA * l.g.L) % 4 == 0 &&
         (uintptr_t)obs % 16 == 0;
}
static int enqueue_fused(const wh_launch& l, void (*fk)(StepParams, float*), float* obs) {
  hipLaunchKernelGGL(fk, grid_for(l.a.B), dim3(2 * BT), 0, l.stream, l.a, obs);
  return hip_err(hipGetLastError());
}

// wh_vector_step and its twins: the step, then the rows of every env (stepped or not) as f32
// (c.obs), as the policy network's fragment-order operand (c.xfrag), or not at all.  The lane-per-env
// f32 form takes one launch when it may: the fast k_sampler instance when the step resolved to the
// fast kernel (every env stepped in ascending order, no metrics, auto-reset: RLlib's common case),
// else the generic one.  The operand form keeps the two launches (k_sampler writing the operand
// from its images ran 1.8 % slower per policy step, profiles/r05_vsx_ab.txt: the operand's per-byte
// gathers at 8 waves per CU against k_observe's full occupancy), and so does the wide step.
static int vector_step(const StepCall& c, void* stream) {
  wh_launch l;
  int rc = resolve_step(c, stream, &l);
  if (rc || c.B == 0) return rc;
  if (c.lanes == 1 && c.obs) {
    void (*fk)(StepParams, float*) =
        (l.kern == l.k->step_fast[0] && l.k->sampler[0]) ? l.k->sampler[0] : l.k->vsampler[c.order ? 1 : 0];
    if (rows_fusable(l, fk, c.obs)) return enqueue_fused(l, fk, c.obs);
  }
  rc = enqueue(l);
  if (rc || (!c.obs && !c.xfrag)) return rc;
  return observe_launch(l.g, l.k, l.a.tables, c.B, c.state, c.obs, c.xfrag, stream);
}

// One sampler step: one launch (k_sampler: the fused rollout's step, then the rows) when the fast
// step instance applies and the rows may be fused; otherwise the step launch and k_observe.
static int sampler_step(const StepCall& c, void* stream) {
  wh_launch l;
  int rc = resolve_step(c, stream, &l);
  if (rc || c.B == 0) return rc;
  if (fast_step(l, c.policy) && rows_fusable(l, l.k->sampler[c.policy], c.obs))
    return enqueue_fused(l, l.k->sampler[c.policy], c.obs);
  rc = enqueue(l);
  if (rc || !c.obs) return rc;
  return observe_launch(l.g, l.k, l.a.tables, c.B, c.state, c.obs, nullptr, stream);
}

extern "C" {

int wh_step(const wh_config* cfg, int64_t B, uint32_t* state, const int32_t* actions,
            const int32_t* order, int32_t order_len, float* rewards, uint8_t* dones, const int32_t* regen,
            int32_t* n_inactive, int32_t phase, uint64_t seed, int64_t env_offset, void* stream) {
  StepCall c;
  const int rc = wh_abi::step_call(&c, cfg, B, state, actions, order, order_len, rewards, dones, regen, n_inactive,
                                   phase, seed, env_offset, 1);
  return rc ? rc : launch_step(c, stream);
}

int wh_policy(const wh_config* cfg, int64_t B, const uint32_t* state, int32_t policy, float p,
              int32_t* actions, uint64_t seed, int64_t env_offset, void* stream) {
  StepCall c;
  const int rc = wh_abi::policy_call(&c, cfg, B, state, policy, p, actions, seed, env_offset);
  return rc ? rc : launch_step(c, stream);
}

int wh_rollout_wide(const wh_config* cfg, int64_t B, uint32_t* state, int32_t steps, int32_t policy, float p,
                    float* rewards, uint8_t* dones, float* returns, const wh_episode_stats* stats,
                    int32_t autoreset, int32_t variable_n, uint64_t seed, int64_t env_offset, int32_t lanes,
                    void* stream) {
  StepCall c;
  const int rc = wh_abi::rollout_call(&c, cfg, B, state, steps, policy, p, rewards, dones, returns, stats, autoreset,
                                      variable_n, seed, env_offset, lanes);
  return rc ? rc : launch_step(c, stream);
}

int wh_rollout(const wh_config* cfg, int64_t B, uint32_t* state, int32_t steps, int32_t policy,
               float p, float* rewards, uint8_t* dones, float* returns, const wh_episode_stats* stats,
               int32_t autoreset, int32_t variable_n, uint64_t seed, int64_t env_offset, void* stream) {
  return wh_rollout_wide(cfg, B, state, steps, policy, p, rewards, dones, returns, stats, autoreset, variable_n, seed,
                         env_offset, 1, stream);
}

int wh_rollout_prepare(const wh_config* cfg, int64_t B, uint32_t* state, int32_t steps, int32_t policy,
                       float p, float* rewards, uint8_t* dones, float* returns, const wh_episode_stats* stats,
                       int32_t autoreset, int32_t variable_n, uint64_t seed, int64_t env_offset, void* stream,
                       wh_launch** out) {
  if (!out) return WH_EINVAL;
  *out = nullptr;
  StepCall c;
  int rc = wh_abi::rollout_call(&c, cfg, B, state, steps, policy, p, rewards, dones, returns, stats, autoreset,
                                variable_n, seed, env_offset, 1);
  if (rc) return rc;
  wh_launch* l = new (std::nothrow) wh_launch;
  if (!l) return WH_EINVAL;
  rc = resolve_step(c, stream, l);
  if (rc) {
    delete l;
    return rc;
  }
  {
    std::lock_guard<std::mutex> lk(g_launch_mu);
    g_launches.insert(l);
  }
  *out = l;
  return WH_OK;
}

int wh_launch_run(const wh_launch* l) { return launch_live(l) ? enqueue(*l) : WH_EINVAL; }

int wh_launch_run_timed(const wh_launch* l, void* start_event, void* stop_event) {
  if (!launch_live(l)) return WH_EINVAL;
  if (l->a.B == 0) return WH_OK;
  StepParams a = l->a;
  void* args[] = {&a};
  return hip_err(hipExtLaunchKernel(reinterpret_cast<const void*>(l->kern), l->grid, dim3(BT), args, 0,
                                    l->stream, (hipEvent_t)start_event, (hipEvent_t)stop_event, 0));
}

int wh_launch_free(wh_launch* l) {
  if (!l) return WH_OK;
  {
    std::lock_guard<std::mutex> lk(g_launch_mu);
    if (!g_launches.erase(l)) return WH_EINVAL;   // not a live handle: never prepared, or freed already
  }
  delete l;
  return WH_OK;
}

int wh_observe(const wh_config* cfg, int64_t B, const uint32_t* state, float* obs, void* stream) {
  return observe_impl(cfg, B, state, obs, nullptr, stream);
}

int wh_observe_x(const wh_config* cfg, int64_t B, const uint32_t* state, float* obs, void* xfrag, void* stream) {
  return observe_impl(cfg, B, state, obs, xfrag, stream);
}

int wh_vector_step(const wh_config* cfg, int64_t B, uint32_t* state, const int32_t* actions,
                   const int32_t* order, int32_t order_len, const uint8_t* mask, float* rewards, uint8_t* dones,
                   float* obs, const wh_episode_stats* stats, int32_t autoreset, int32_t variable_n,
                   uint64_t seed, int64_t env_offset, void* stream) {
  StepCall c;
  const int rc = wh_abi::vector_step_call(&c, cfg, B, state, actions, order, order_len, mask, rewards, dones, obs,
                                          nullptr, false, stats, autoreset, variable_n, seed, env_offset, 1);
  return rc ? rc : vector_step(c, stream);
}

// wh_vector_step with the rows written as the policy network's fragment-order operand (the policy
// route, scripts/rollout.py:72 -> env.step)
int wh_vector_step_x(const wh_config* cfg, int64_t B, uint32_t* state, const int32_t* actions,
                     const int32_t* order, int32_t order_len, const uint8_t* mask, float* rewards, uint8_t* dones,
                     void* xfrag, const wh_episode_stats* stats, int32_t autoreset, int32_t variable_n,
                     uint64_t seed, int64_t env_offset, void* stream) {
  StepCall c;
  const int rc = wh_abi::vector_step_call(&c, cfg, B, state, actions, order, order_len, mask, rewards, dones, nullptr,
                                          xfrag, true, stats, autoreset, variable_n, seed, env_offset, 1);
  return rc ? rc : vector_step(c, stream);
}

int wh_sampler_step(const wh_config* cfg, int64_t B, uint32_t* state, int32_t policy, float p,
                    float* rewards, uint8_t* dones, float* obs, const wh_episode_stats* stats,
                    int32_t variable_n, uint64_t seed, int64_t env_offset, void* stream) {
  StepCall c;
  const int rc = wh_abi::sampler_step_call(&c, cfg, B, state, nullptr, false, policy, p, rewards, dones, obs, stats,
                                           variable_n, seed, env_offset);
  return rc ? rc : sampler_step(c, stream);
}

int wh_sampler_rollout(const wh_config* cfg, int64_t B, uint32_t* state, int32_t steps, int32_t policy, float p,
                       float* rewards, uint8_t* dones, float* obs, const wh_episode_stats* stats, int32_t variable_n,
                       uint64_t seed, int64_t env_offset, void* stream) {
  StepCall c;
  int rc = wh_abi::sampler_rollout_call(&c, cfg, B, state, steps, policy, p, rewards, dones, obs, stats, variable_n,
                                        seed, env_offset);
  if (rc) return rc;
  wh_launch l;
  rc = resolve_step(c, stream, &l);
  if (rc || B == 0 || steps == 0) return rc;
  void (*fk)(StepParams, float*) = steps == 1 ? l.k->sampler[policy] : l.k->sampler_multi[policy];
  if (fast_step(l, policy) && rows_fusable(l, fk, obs)) return enqueue_fused(l, fk, obs);
  // otherwise: the same steps one launch (pair) at a time
  c.steps = 1;
  for (int32_t t = 0; t < steps && rc == WH_OK; ++t) {
    rc = sampler_step(c, stream);
    if (c.rewards) c.rewards += B * c.g.NA;
    if (c.dones) c.dones += B;
    c.obs += B * c.g.NA * c.g.L;
  }
  return rc;
}

int wh_sampler_step_to(const wh_config* cfg, int64_t B, const uint32_t* state_in, uint32_t* state_out,
                       int32_t policy, float p, float* rewards, uint8_t* dones, const wh_episode_stats* stats,
                       int32_t variable_n, uint64_t seed, int64_t env_offset, void* stream) {
  StepCall c;
  const int rc = wh_abi::sampler_step_call(&c, cfg, B, state_in, state_out, true, policy, p, rewards, dones, nullptr,
                                           stats, variable_n, seed, env_offset);
  return rc ? rc : launch_step(c, stream);
}

// ---- the 16-lanes-per-env execution form (csrc/step_wide.h).  lanes == WH_WIDE_LANES runs
// k_step_wide; lanes == 1 is the lane-per-env entry point itself (ascending order, whole step).
int wh_step_wide(const wh_config* cfg, int64_t B, uint32_t* state, const int32_t* actions, float* rewards,
                 uint8_t* dones, const int32_t* regen, int32_t* n_inactive, uint64_t seed, int64_t env_offset,
                 int32_t lanes, void* stream) {
  StepCall c;
  const int rc = wh_abi::step_call(&c, cfg, B, state, actions, nullptr, 0, rewards, dones, regen, n_inactive,
                                   WH_PHASE_ALL, seed, env_offset, lanes);
  return rc ? rc : launch_step(c, stream);
}

// the wide step launch, then k_observe: two launches
int wh_vector_step_wide(const wh_config* cfg, int64_t B, uint32_t* state, const int32_t* actions,
                        const uint8_t* mask, float* rewards, uint8_t* dones, float* obs,
                        const wh_episode_stats* stats, int32_t autoreset, int32_t variable_n, uint64_t seed,
                        int64_t env_offset, int32_t lanes, void* stream) {
  StepCall c;
  const int rc = wh_abi::vector_step_call(&c, cfg, B, state, actions, nullptr, 0, mask, rewards, dones, obs, nullptr,
                                          false, stats, autoreset, variable_n, seed, env_offset, lanes);
  return rc ? rc : vector_step(c, stream);
}

// ---- replay ring (csrc/replay.h).  abi_args.h has checked the call; B > 0 (and M > 0) here.
int wh_replay_put(const wh_config* cfg, int64_t B, const wh_replay_ring* ring, int64_t slot, int32_t stage,
                  const uint32_t* state, const int32_t* actions, const float* rewards, const uint8_t* dones,
                  void* stream) {
  Geometry g;
  int rc = wh_abi::replay_put_call(&g, cfg, B, ring, slot, stage, state, actions, rewards, dones);
  if (rc) return rc;
  const Kernels* k = pick(g);
  if (!k) return WH_ENOTSUP;
  if (B == 0) return WH_OK;
  const int64_t step = slot * B;
  PutParams a{state, ring->states + (2 * step + (int64_t)stage * B) * g.words, B, g.words, g.NA,
              stage == 0 ? actions : nullptr, stage == 0 ? ring->actions + step * g.NA : nullptr,
              stage == 1 ? rewards : nullptr, stage == 1 ? ring->rewards + step * g.NA : nullptr,
              stage == 1 ? dones : nullptr, stage == 1 ? ring->dones + step : nullptr};
  hipLaunchKernelGGL(k->replay_put, grid_for(B), dim3(BT), 0, (hipStream_t)stream, a);
  return hip_err(hipGetLastError());
}

int wh_replay_gather(const wh_config* cfg, int64_t B, const wh_replay_ring* ring, int64_t filled, int64_t M,
                     const int64_t* idx, uint64_t seed, uint64_t draw, const wh_replay_batch* batch, void* stream) {
  Geometry g;
  int rc = wh_abi::replay_gather_call(&g, cfg, B, ring, filled, M, batch);
  if (rc) return rc;
  const Kernels* k;
  const uint32_t* tab;
  const bool empty = B == 0 || M == 0;
  rc = locate(g, empty ? 0 : B, stream, &k, &tab);
  if (rc || empty) return rc;
  const bool frags = batch->xfrag || batch->next_xfrag;
  // samples per workgroup: k_observe's choice for f32 rows of this size (never kObsEB[1], the
  // fragments-only group, whose gather instance is not built)
  const int sel = obs_group_sel(g, true, frags);
  const int eb = kObsEB[sel];
  const int64_t groups = (M + eb - 1) / eb;
  const bool next = batch->next_obs || batch->next_xfrag || batch->next_state;
  if (groups * 2 > 0x7FFFFFFF) return WH_EINVAL;
  GatherParams a{};
  a.states = ring->states;
  a.r_actions = ring->actions;
  a.r_rewards = ring->rewards;
  a.r_dones = ring->dones;
  a.B = B;
  a.filled = filled;
  a.M = M;
  a.idx = idx;
  a.k0 = wh_abi::lo32(seed);
  a.k1 = wh_abi::hi32(seed);
  a.d0 = wh_abi::lo32(draw);
  a.d1 = wh_abi::hi32(draw);
  a.na = g.NA;
  a.words = g.words;
  a.quads = (g.NA * g.L) % 4 == 0;
  a.groups = (unsigned)groups;
  a.tables = tab;
  a.obs[0] = batch->obs;
  a.obs[1] = batch->next_obs;
  a.xfrag[0] = static_cast<uint4*>(batch->xfrag);
  a.xfrag[1] = static_cast<uint4*>(batch->next_xfrag);
  a.state[0] = batch->state;
  a.state[1] = batch->next_state;
  a.actions = batch->actions;
  a.rewards = batch->rewards;
  a.dones = batch->dones;
  a.n = batch->n;
  a.idx_out = batch->idx_out;
  hipLaunchKernelGGL(k->replay_gather[sel], dim3((unsigned)(groups * (next ? 2 : 1))), dim3(BT), 0,
                     (hipStream_t)stream, a);
  return hip_err(hipGetLastError());
}

// `steps` recorded steps in one launch (csrc/step_record.h), then the rows of the final state through
// k_observe: the ring bytes, state, rewards, dones, metrics and draws of [wh_policy ->] put(0) ->
// wh_vector_step(autoreset = 0) -> put(1) -> wh_reset(mask = dones), `steps` times.
int wh_replay_record(const wh_config* cfg, int64_t B, uint32_t* state, const wh_replay_ring* ring, int64_t slot,
                     int32_t steps, int32_t policy, float p, const int32_t* actions, float* rewards, uint8_t* dones,
                     float* obs, void* xfrag, const wh_episode_stats* stats, int32_t variable_n, uint64_t seed,
                     int64_t env_offset, void* stream) {
  StepCall c;
  int rc = wh_abi::replay_record_call(&c, cfg, B, state, ring, slot, steps, policy, p, actions, rewards, dones, obs,
                                      xfrag, stats, variable_n, seed, env_offset);
  if (rc) return rc;
  const Kernels* k;
  const uint32_t* tab;
  const bool empty = B == 0 || steps == 0;
  rc = locate(c.g, empty ? 0 : B, stream, &k, &tab);
  if (rc || empty) return rc;
  const RecordParams a{step_params(c, tab), ring->states, ring->actions, ring->rewards, ring->dones, slot,
                       ring->capacity, c.g.words};
  hipLaunchKernelGGL(k->step_record[policy], grid_for(B), dim3(BT), 0, (hipStream_t)stream, a);
  rc = hip_err(hipGetLastError());
  if (rc || (!obs && !xfrag)) return rc;
  return observe_launch(c.g, k, tab, B, state, obs, xfrag, stream);
}

// ---- replay priorities (csrc/prio.h).  abi_args.h has checked the call.
static PrioTree prio_tree_of(const wh_replay_prio* tree, const wh_abi::PrioShape& s) {
  PrioTree t{};
  t.leaf = tree->leaf;
  t.node = tree->node;
  t.max_q = tree->max_q;
  t.count = tree->count;
  t.levels = s.levels;
  for (int k = 0; k <= s.levels; ++k) {
    t.n[k] = s.n[k];
    t.off[k] = s.off[k];
  }
  return t;
}

int wh_replay_prio_query(int64_t count, int64_t* leaf_words, int64_t* node_words, int32_t* levels) {
  return wh_abi::prio_query(count, leaf_words, node_words, levels);
}

int wh_replay_prio_fill(const wh_replay_prio* tree, int64_t first, int64_t n, int32_t mode, uint32_t q,
                        void* stream) {
  wh_abi::PrioShape s;
  const int rc = wh_abi::prio_fill_call(&s, tree, first, n, mode, q);
  if (rc || n == 0) return rc;
  PrioFillParams a{prio_tree_of(tree, s), first, first + n, first & ~(int64_t)(BT - 1), mode, q};
  hipLaunchKernelGGL(k_prio_fill, grid_for(a.end - a.base), dim3(BT), 0, (hipStream_t)stream, a);
  return hip_err(hipGetLastError());
}

int wh_replay_prio_update(const wh_replay_prio* tree, int64_t M, const int64_t* idx, const float* p,
                          void* stream) {
  wh_abi::PrioShape s;
  const int rc = wh_abi::prio_update_call(&s, tree, M, idx, p);
  if (rc || M == 0) return rc;
  if ((M + BT - 1) / BT > 0x7FFFFFFF) return WH_EINVAL;
  PrioUpdateParams a{prio_tree_of(tree, s), M, idx, p, 0};
  hipLaunchKernelGGL(k_prio_update, grid_for(M), dim3(BT), 0, (hipStream_t)stream, a);
  a.phase = 1;
  hipLaunchKernelGGL(k_prio_update, grid_for(M), dim3(BT), 0, (hipStream_t)stream, a);
  return hip_err(hipGetLastError());
}

int wh_replay_prio_sample(const wh_replay_prio* tree, int64_t M, const uint64_t* u, uint64_t seed, uint64_t draw,
                          int64_t* idx_out, uint32_t* q_out, uint64_t* total_out, void* stream) {
  wh_abi::PrioShape s;
  const int rc = wh_abi::prio_sample_call(&s, tree, M, idx_out);
  if (rc || M == 0) return rc;
  const int64_t groups = (M + BT / 16 - 1) / (BT / 16);
  if (groups > 0x7FFFFFFF) return WH_EINVAL;
  PrioSampleParams a{prio_tree_of(tree, s), M, u, wh_abi::lo32(seed), wh_abi::hi32(seed), wh_abi::lo32(draw),
                     wh_abi::hi32(draw), idx_out, q_out, total_out};
  hipLaunchKernelGGL(k_prio_sample, dim3((unsigned)groups), dim3(BT), 0, (hipStream_t)stream, a);
  return hip_err(hipGetLastError());
}

// ---- SAC TD targets (csrc/sac.h).  abi_args.h has checked the call.
int wh_sac_td(int64_t M, int32_t NA, const wh_sac_td_args* a, void* stream) {
  const int rc = wh_abi::sac_td_call(M, NA, a);
  if (rc || M == 0) return rc;
  const int32_t spw = BT / NA;   // whole samples per workgroup
  const int64_t groups = (M + spw - 1) / spw;
  if (groups > 0x7FFFFFFF) return WH_EINVAL;
  const SacParams p{*a, M, NA, spw};
  hipLaunchKernelGGL(k_sac_td, dim3((unsigned)groups), dim3(BT), 0, (hipStream_t)stream, p);
  return hip_err(hipGetLastError());
}

int wh_sac_td_la(int64_t M, int32_t NA, const wh_sac_td_args* a, const float* log_alpha, void* stream) {
  const int rc = wh_abi::sac_td_la_call(M, NA, a, log_alpha);
  if (rc || M == 0) return rc;
  const int32_t spw = BT / NA;
  const int64_t groups = (M + spw - 1) / spw;
  if (groups > 0x7FFFFFFF) return WH_EINVAL;
  const SacParams p{*a, M, NA, spw};
  hipLaunchKernelGGL(k_sac_la_td, dim3((unsigned)groups), dim3(BT), 0, (hipStream_t)stream, p, log_alpha);
  return hip_err(hipGetLastError());
}

// ---- SAC losses (csrc/sac_loss.h): one launch, and for more than one workgroup the launch that adds
// their partial sums
int wh_sac_loss_query(int64_t M, int32_t NA, int64_t* work_bytes) { return wh_abi::sac_loss_query_call(M, NA, work_bytes); }

int wh_sac_loss(int64_t M, int32_t NA, const wh_sac_loss_args* a, void* stream) {
  const int rc = wh_abi::sac_loss_call(M, NA, a);
  if (rc || M == 0) return rc;
  const int64_t groups = wh_abi::sac_loss_groups(M, NA);
  if (groups > 0x7FFFFFFF) return WH_EINVAL;
  const SacLossParams p{*a, M, NA, BT / NA};
  hipLaunchKernelGGL(k_sac_loss, dim3((unsigned)groups), dim3(BT), 0, (hipStream_t)stream, p);
  if (groups > 1) {
    const SacLossFinishParams f{static_cast<const float*>(a->work), groups, a->log_alpha, a->scale, a->stats};
    hipLaunchKernelGGL(k_sac_loss_finish, dim3(1), dim3(BT), 0, (hipStream_t)stream, f);
  }
  return hip_err(hipGetLastError());
}

// ---- Adam (csrc/adam.h): the segment table and every segment's first workgroup go in the argument
static int adam_params(int32_t nseg, const wh_adam_seg* segs, AdamParams* p, int64_t* groups_out) {
  int64_t groups = 0;
  for (int32_t s = 0; s < nseg; ++s) {
    p->seg[s] = segs[s];
    p->start[s] = (uint32_t)groups;
    groups += (segs[s].count + ADAM_CHUNK - 1) / ADAM_CHUNK;
    if (groups > 0x7FFFFFFF) return WH_EINVAL;
  }
  p->start[nseg] = (uint32_t)groups;
  p->nseg = nseg;
  *groups_out = groups;
  return WH_OK;
}

int wh_adam_step(int32_t nseg, const wh_adam_seg* segs, const wh_adam_hyper* h, void* stream) {
  int rc = wh_abi::adam_call(nseg, segs, h);
  if (rc || nseg == 0) return rc;
  AdamParams p{};
  int64_t groups = 0;
  if ((rc = adam_params(nseg, segs, &p, &groups))) return rc;
  p.h = *h;
  if (groups == 0) return WH_OK;
  hipLaunchKernelGGL(k_adam, dim3((unsigned)groups), dim3(BT), 0, (hipStream_t)stream, p);
  return hip_err(hipGetLastError());
}

// the tick, then -- in stream order -- the step that reads the table the tick wrote
int wh_adam_step_clock(int32_t nseg, const wh_adam_seg* segs, wh_adam_clock* clock, double lr, double beta1,
                       double beta2, double eps, void* stream) {
  int rc = wh_abi::adam_clock_call(nseg, segs, clock);
  if (rc) return rc;
  AdamParams p{};
  int64_t groups = 0;
  if ((rc = adam_params(nseg, segs, &p, &groups))) return rc;   // (before the tick: a refused call changes nothing)
  const AdamTickParams tick{clock, lr, beta1, beta2, eps};
  hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(64), 0, (hipStream_t)stream, tick);
  if (groups > 0)
    hipLaunchKernelGGL(k_adam_clock, dim3((unsigned)groups), dim3(BT), 0, (hipStream_t)stream, p, clock);
  return hip_err(hipGetLastError());
}

}  // extern "C"
