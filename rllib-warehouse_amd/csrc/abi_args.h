// abi_args.h -- the argument rules of the C ABI (include/warehouse_amd.h), written once for the two
// libraries behind it: the gfx950 library (warehouse_amd.hip) and the host engine (host_engine.cpp).
// Plain C++17, no HIP.  What is here is a property of the ABI, not of a back end: which configs
// are valid and the sizes that follow from one, which option values an entry point refuses, and a
// step-family call checked and reduced to one struct (StepCall) that a back end then runs.  What a
// back end cannot run -- no kernel instance for a geometry, racks that overlap, the host engine's
// 64-point sets -- it refuses itself, after these checks.
//
// Order of the checks, hence the code returned when several things are wrong at once: `lanes`, the
// entry point's own options and required pointers (WH_EINVAL), the config (WH_EINVAL, or
// WH_ENOTSUP for racks on the border), the state pointer, the order-row width, B < 0 (WH_EINVAL);
// then the back end's refusals.  Only the pointer checks depend on the batch: a bad option or config
// is refused for an empty batch (B = 0 or steps = 0) like for a full one.
#pragma once
#include <stdint.h>

#include "warehouse_amd.h"

namespace wh_abi {

// ----------------------------------------------------------------------------- config
struct Shape {   // a valid wh_config and the sizes that follow from it
  int D, R, NR, NA, T, W;
  int P, DP;     // pickup points 4 NR^2 (core.py:171-175), delivery points 4 (D - 4) (core.py:178-188)
  int L, words;  // floats per observation row 9 R + 1, packed state words per env
  int racks[WH_MAX_RACKS];
};

inline int check_config(const wh_config* c, Shape* g) {
  if (!c) return WH_EINVAL;
  g->D = c->area_dimension;
  g->R = c->num_requests;
  g->NR = c->num_racks;
  g->NA = c->agent_slots;
  g->T = c->episode_duration;
  g->W = c->pickup_wait_duration;
  if (g->NR < 1 || g->NR > WH_MAX_RACKS || g->D < 5 || g->D > 32) return WH_EINVAL;
  g->P = 4 * g->NR * g->NR;
  g->DP = 4 * (g->D - 4);
  if (g->NA < 1 || g->NA > g->R || g->R > g->P || g->R > g->DP) return WH_EINVAL;
  if (g->W < 1 || g->W > 255 || g->T < 0) return WH_EINVAL;
  for (int i = 0; i < g->NR; ++i) {
    g->racks[i] = c->racks[i];
    if (c->racks[i] < 2 || c->racks[i] > g->D - 2) return WH_ENOTSUP;   // pickups must be interior
  }
  g->L = 9 * g->R + 1;
  g->words = 2 + g->NA + 2 * (g->P / 4);
  return WH_OK;
}

// ----------------------------------------------------------------------------- option values
inline bool policy_ok(int32_t policy) { return policy == WH_POLICY_GREEDY || policy == WH_POLICY_RANDOM; }
inline bool p_ok(float p) { return p >= 0.0f && p <= 1.0f; }   // (a NaN fails both comparisons)
inline bool phase_ok(int32_t phase) { return phase >= WH_PHASE_ALL && phase <= WH_PHASE_REGEN; }
inline bool lanes_ok(int32_t lanes) { return lanes == 1 || lanes == WH_WIDE_LANES; }
// episode bins are folded from the per-env return accumulator: bins without it are refused
inline bool stats_ok(const wh_episode_stats* st) {
  return !st || st->episode_return || (!st->return_sum && !st->episodes && !st->return_min && !st->return_max);
}
// entries per order row: 0 = agent_slots, else 1 .. 4 * agent_slots (every key form of every agent,
// core.py:280); -1 = refused
inline int order_width(const Shape& g, int32_t order_len) {
  if (order_len == 0) return g.NA;
  return (order_len >= 1 && order_len <= 4 * g.NA) ? order_len : -1;
}

// ----------------------------------------------------------------------------- a step-family call
constexpr int32_t POLICY_EXTERNAL = 0;   // StepCall::policy of the entries that take actions
constexpr int32_t PHASE_POLICY = 3;      // StepCall::phase of wh_policy: actions out, no transition

struct StepCall {
  Shape g;
  int64_t B;
  uint32_t* state;
  int32_t lanes;            // 1, or WH_WIDE_LANES (wh_*_wide)
  int32_t policy;           // POLICY_EXTERNAL, WH_POLICY_GREEDY, WH_POLICY_RANDOM
  float p;
  const int32_t* actions;
  const int32_t* order;
  int32_t ol;               // entries per order row, resolved (1 .. 4 * NA)
  const uint8_t* mask;
  float* rewards;
  uint8_t* dones;
  float* returns;
  const int32_t* regen;
  int32_t* n_inactive;
  int32_t* actions_out;     // wh_policy
  float* obs;
  void* xfrag;              // wh_vector_step_x
  uint32_t* state_out;      // wh_sampler_step_to
  const wh_episode_stats* stats;
  const wh_replay_ring* ring;   // wh_replay_record: every step recorded, step k into slot (slot + k) % capacity
  int64_t slot;
  int32_t steps, phase, autoreset, variable_n;   // (the two flags as 0 / 1)
  uint64_t seed;
  int64_t env_offset;
};

// the head and the tail every family shares
inline void begin(StepCall* c, int64_t B, const uint32_t* state, uint64_t seed, int64_t env_offset) {
  *c = StepCall{};
  c->B = B;
  c->state = const_cast<uint32_t*>(state);
  c->lanes = 1;
  c->steps = 1;
  c->phase = WH_PHASE_ALL;
  c->seed = seed;
  c->env_offset = env_offset;
}
inline int finish(StepCall* c, const wh_config* cfg) {
  const int rc = check_config(cfg, &c->g);
  if (rc) return rc;
  if (c->B > 0 && !c->state) return WH_EINVAL;
  c->ol = order_width(c->g, c->ol);
  return (c->ol < 0 || c->B < 0) ? WH_EINVAL : WH_OK;
}
inline void rollout_options(StepCall* c, int32_t steps, int32_t policy, float p, float* rewards, uint8_t* dones,
                            const wh_episode_stats* stats, int32_t autoreset, int32_t variable_n) {
  c->steps = steps;
  c->policy = policy;
  c->p = p;
  c->rewards = rewards;
  c->dones = dones;
  c->stats = stats;
  c->autoreset = autoreset ? 1 : 0;
  c->variable_n = variable_n ? 1 : 0;
}

// wh_step, wh_step_wide (order = NULL, the whole step)
inline int step_call(StepCall* c, const wh_config* cfg, int64_t B, uint32_t* state, const int32_t* actions,
                     const int32_t* order, int32_t order_len, float* rewards, uint8_t* dones, const int32_t* regen,
                     int32_t* n_inactive, int32_t phase, uint64_t seed, int64_t env_offset, int32_t lanes) {
  if (!lanes_ok(lanes) || !phase_ok(phase)) return WH_EINVAL;
  if (B > 0 && phase != WH_PHASE_REGEN && !actions) return WH_EINVAL;
  begin(c, B, state, seed, env_offset);
  c->lanes = lanes;
  c->actions = actions;
  c->order = order;
  c->ol = order_len;
  c->rewards = rewards;
  c->dones = dones;
  c->regen = regen;
  c->n_inactive = n_inactive;
  c->phase = phase;
  return finish(c, cfg);
}

// wh_policy
inline int policy_call(StepCall* c, const wh_config* cfg, int64_t B, const uint32_t* state, int32_t policy, float p,
                       int32_t* actions, uint64_t seed, int64_t env_offset) {
  if (!policy_ok(policy) || (B > 0 && !actions) || !p_ok(p)) return WH_EINVAL;
  begin(c, B, state, seed, env_offset);
  c->policy = policy;
  c->p = p;
  c->actions_out = actions;
  c->steps = 0;
  c->phase = PHASE_POLICY;
  return finish(c, cfg);
}

// wh_rollout, wh_rollout_prepare, wh_rollout_wide
inline int rollout_call(StepCall* c, const wh_config* cfg, int64_t B, uint32_t* state, int32_t steps, int32_t policy,
                        float p, float* rewards, uint8_t* dones, float* returns, const wh_episode_stats* stats,
                        int32_t autoreset, int32_t variable_n, uint64_t seed, int64_t env_offset, int32_t lanes) {
  if (!lanes_ok(lanes) || !policy_ok(policy) || steps < 0 || !p_ok(p) || !stats_ok(stats)) return WH_EINVAL;
  begin(c, B, state, seed, env_offset);
  rollout_options(c, steps, policy, p, rewards, dones, stats, autoreset, variable_n);
  c->lanes = lanes;
  c->returns = returns;
  return finish(c, cfg);
}

// wh_vector_step, wh_vector_step_x (rows to `xfrag`, required), wh_vector_step_wide (order = NULL)
inline int vector_step_call(StepCall* c, const wh_config* cfg, int64_t B, uint32_t* state, const int32_t* actions,
                            const int32_t* order, int32_t order_len, const uint8_t* mask, float* rewards,
                            uint8_t* dones, float* obs, void* xfrag, bool to_xfrag, const wh_episode_stats* stats,
                            int32_t autoreset, int32_t variable_n, uint64_t seed, int64_t env_offset, int32_t lanes) {
  if (!lanes_ok(lanes) || (B > 0 && !actions)) return WH_EINVAL;
  if (to_xfrag && ((B > 0 && !xfrag) || (uintptr_t)xfrag % 16 != 0)) return WH_EINVAL;
  if (!stats_ok(stats)) return WH_EINVAL;
  begin(c, B, state, seed, env_offset);
  rollout_options(c, 1, POLICY_EXTERNAL, 0.0f, rewards, dones, stats, autoreset, variable_n);
  c->lanes = lanes;
  c->actions = actions;
  c->order = order;
  c->ol = order_len;
  c->mask = mask;
  c->obs = obs;
  c->xfrag = xfrag;
  return finish(c, cfg);
}

// wh_sampler_step, wh_sampler_step_to (the state written to `state_out`, required)
inline int sampler_step_call(StepCall* c, const wh_config* cfg, int64_t B, const uint32_t* state, uint32_t* state_out,
                             bool to_state_out, int32_t policy, float p, float* rewards, uint8_t* dones, float* obs,
                             const wh_episode_stats* stats, int32_t variable_n, uint64_t seed, int64_t env_offset) {
  if (!policy_ok(policy) || !p_ok(p) || !stats_ok(stats)) return WH_EINVAL;
  if (to_state_out && B > 0 && !state_out) return WH_EINVAL;
  begin(c, B, state, seed, env_offset);
  rollout_options(c, 1, policy, p, rewards, dones, stats, 1, variable_n);
  c->obs = obs;
  c->state_out = state_out;
  return finish(c, cfg);
}

// wh_sampler_rollout: `steps` sampler steps, the rows of every step kept
inline int sampler_rollout_call(StepCall* c, const wh_config* cfg, int64_t B, uint32_t* state, int32_t steps,
                                int32_t policy, float p, float* rewards, uint8_t* dones, float* obs,
                                const wh_episode_stats* stats, int32_t variable_n, uint64_t seed, int64_t env_offset) {
  if (!policy_ok(policy) || steps < 0 || !p_ok(p) || !stats_ok(stats)) return WH_EINVAL;
  if (B > 0 && steps > 0 && !obs) return WH_EINVAL;
  begin(c, B, state, seed, env_offset);
  rollout_options(c, steps, policy, p, rewards, dones, stats, 1, variable_n);
  c->obs = obs;
  return finish(c, cfg);
}

// ----------------------------------------------------------------------------- pack, reset, observe
// The config first, as everywhere.  A *_call that answers WH_OK for an empty batch (B == 0) has
// looked at no pointer: the back end returns after its own refusals, without running anything.

// a 64-bit seed or draw counter as the two 32-bit words of a Philox key or counter
inline uint32_t lo32(uint64_t v) { return (uint32_t)(v & 0xFFFFFFFFu); }
inline uint32_t hi32(uint64_t v) { return (uint32_t)(v >> 32); }

// wh_pack, wh_unpack (`state` and the eight canonical arrays, all required): the empty batch is
// accepted before B < 0 and the pointers are looked at
inline int pack_call(Shape* g, const wh_config* cfg, int64_t B, const void* state, const void* pos,
                     const void* agent_target, const void* pickup_target, const void* pickup_timer, const void* t,
                     const void* n, const void* fresh, const void* episode) {
  const int rc = check_config(cfg, g);
  if (rc || B == 0) return rc;
  return (B < 0 || !pos || !agent_target || !pickup_target || !pickup_timer || !t || !n || !fresh || !episode || !state)
             ? WH_EINVAL : WH_OK;
}

// wh_reset: injected draws come whole (spawn, pickups, targets; n is optional)
inline int reset_call(Shape* g, const wh_config* cfg, int64_t B, const uint32_t* state, const wh_reset_draws* draws) {
  const int rc = check_config(cfg, g);
  if (rc) return rc;
  if (B < 0) return WH_EINVAL;
  if (B == 0) return WH_OK;
  if (!state) return WH_EINVAL;
  return (draws && (!draws->spawn || !draws->pickups || !draws->targets)) ? WH_EINVAL : WH_OK;
}

// wh_observe (xfrag = NULL), wh_observe_x (rows to `obs`, to the 16-byte aligned `xfrag`, or both)
inline int observe_call(Shape* g, const wh_config* cfg, int64_t B, const uint32_t* state, const float* obs,
                        const void* xfrag) {
  const int rc = check_config(cfg, g);
  if (rc) return rc;
  if (B < 0) return WH_EINVAL;
  if (B == 0) return WH_OK;
  return (!state || (!obs && !xfrag) || (uintptr_t)xfrag % 16 != 0) ? WH_EINVAL : WH_OK;
}

// ----------------------------------------------------------------------------- replay ring
// The same order as the step family: the entry point's own options and required pointers, the
// config, the state pointer (put) or the alignment that depends on the config (gather), B < 0.
inline bool ring_ok(const wh_replay_ring* ring) { return ring && ring->capacity >= 1; }

// wh_replay_put
inline int replay_put_call(Shape* g, const wh_config* cfg, int64_t B, const wh_replay_ring* ring, int64_t slot,
                           int32_t stage, const uint32_t* state, const int32_t* actions, const float* rewards,
                           const uint8_t* dones) {
  if (!ring_ok(ring) || slot < 0 || slot >= ring->capacity || (stage != 0 && stage != 1)) return WH_EINVAL;
  if (B > 0) {
    if (!ring->states) return WH_EINVAL;
    if (stage == 0 && (!ring->actions || !actions)) return WH_EINVAL;
    if (stage == 1 && (!ring->rewards || !ring->dones || !rewards || !dones)) return WH_EINVAL;
  }
  const int rc = check_config(cfg, g);
  if (rc) return rc;
  return ((B > 0 && !state) || B < 0) ? WH_EINVAL : WH_OK;
}

// wh_replay_record: `steps` recorded steps (external actions: one), then the rows of the final state
inline int replay_record_call(StepCall* c, const wh_config* cfg, int64_t B, uint32_t* state, const wh_replay_ring* ring,
                              int64_t slot, int32_t steps, int32_t policy, float p, const int32_t* actions,
                              float* rewards, uint8_t* dones, float* obs, void* xfrag, const wh_episode_stats* stats,
                              int32_t variable_n, uint64_t seed, int64_t env_offset) {
  if (!ring_ok(ring) || slot < 0 || slot >= ring->capacity || steps < 0 || steps > ring->capacity) return WH_EINVAL;
  if (policy != POLICY_EXTERNAL && !policy_ok(policy)) return WH_EINVAL;
  if (policy == POLICY_EXTERNAL && steps > 1) return WH_EINVAL;   // one action set, one step
  if (!p_ok(p) || !stats_ok(stats) || (uintptr_t)xfrag % 16 != 0) return WH_EINVAL;
  if (B > 0 && steps > 0) {
    if (!ring->states || !ring->actions || !ring->rewards || !ring->dones) return WH_EINVAL;
    if (policy == POLICY_EXTERNAL && !actions) return WH_EINVAL;
  }
  begin(c, B, state, seed, env_offset);
  rollout_options(c, steps, policy, p, rewards, dones, stats, 1, variable_n);
  c->actions = actions;
  c->obs = obs;
  c->xfrag = xfrag;
  c->ring = ring;
  c->slot = slot;
  return finish(c, cfg);
}

inline bool batch_has_frags(const wh_replay_batch* b) { return b->xfrag || b->next_xfrag; }

// wh_replay_gather
inline int replay_gather_call(Shape* g, const wh_config* cfg, int64_t B, const wh_replay_ring* ring, int64_t filled,
                              int64_t M, const wh_replay_batch* b) {
  if (!ring_ok(ring) || filled < 1 || filled > ring->capacity || M < 0 || !b) return WH_EINVAL;
  if (!b->obs && !b->next_obs && !b->xfrag && !b->next_xfrag && !b->state && !b->next_state && !b->actions &&
      !b->rewards && !b->dones && !b->n && !b->idx_out)
    return WH_EINVAL;
  if (B > 0 && M > 0) {
    if (!ring->states) return WH_EINVAL;
    if ((b->actions && !ring->actions) || (b->rewards && !ring->rewards) || (b->dones && !ring->dones))
      return WH_EINVAL;
  }
  if ((uintptr_t)b->xfrag % 16 != 0 || (uintptr_t)b->next_xfrag % 16 != 0) return WH_EINVAL;
  const int rc = check_config(cfg, g);
  if (rc) return rc;
  if ((g->NA * g->L) % 4 == 0 && ((uintptr_t)b->obs % 16 != 0 || (uintptr_t)b->next_obs % 16 != 0))
    return WH_EINVAL;   // rows written as float4
  return B < 0 ? WH_EINVAL : WH_OK;
}

// ----------------------------------------------------------------------------- replay priorities
// The radix-16 tree of `count` leaves (include/warehouse_amd.h, REPLAY PRIORITIES): level k >= 1
// has n[k] sums and starts at word off[k] of `node`; level `levels` is the root.
constexpr int PRIO_MAX_LEVELS = 8;   // 2^31 leaves: 2^27, 2^23, ... 2^3, 1 sums

struct PrioShape {
  int32_t levels;
  int64_t leaf_words, node_words;
  int64_t n[PRIO_MAX_LEVELS + 1], off[PRIO_MAX_LEVELS + 1];   // [0]: the leaves (off unused)
};

inline int64_t pad16(int64_t n) { return (n + 15) & ~(int64_t)15; }

inline int prio_shape(int64_t count, PrioShape* s) {
  if (count < 1 || count > WH_PRIO_MAX_COUNT) return WH_EINVAL;
  *s = PrioShape{};
  s->n[0] = count;
  s->leaf_words = pad16(count);
  int64_t n = count;
  do {
    n = (n + 15) / 16;
    ++s->levels;
    s->n[s->levels] = n;
    s->off[s->levels] = s->node_words;
    s->node_words += pad16(n);
  } while (n > 1);
  return WH_OK;
}

// wh_replay_prio_query, whole: it asks nothing of a back end
inline int prio_query(int64_t count, int64_t* leaf_words, int64_t* node_words, int32_t* levels) {
  PrioShape s;
  const int rc = prio_shape(count, &s);
  if (rc) return rc;
  if (leaf_words) *leaf_words = s.leaf_words;
  if (node_words) *node_words = s.node_words;
  if (levels) *levels = s.levels;
  return WH_OK;
}

// Required pointers, then the sizes, then M < 0; the pointers of the batch only for M > 0.
inline int prio_tree(const wh_replay_prio* t, PrioShape* s) {
  if (!t || !t->leaf || !t->node || !t->max_q) return WH_EINVAL;
  return prio_shape(t->count, s);
}

// wh_replay_prio_fill
inline int prio_fill_call(PrioShape* s, const wh_replay_prio* t, int64_t first, int64_t n, int32_t mode, uint32_t q) {
  if ((mode != 0 && mode != 1) || (mode == 0 && q > WH_PRIO_MAX)) return WH_EINVAL;
  const int rc = prio_tree(t, s);
  if (rc) return rc;
  return (first < 0 || n < 0 || first > t->count || n > t->count - first) ? WH_EINVAL : WH_OK;
}

// wh_replay_prio_update
inline int prio_update_call(PrioShape* s, const wh_replay_prio* t, int64_t M, const int64_t* idx, const float* p) {
  if (M > 0 && (!idx || !p)) return WH_EINVAL;
  const int rc = prio_tree(t, s);
  if (rc) return rc;
  return M < 0 ? WH_EINVAL : WH_OK;
}

// wh_replay_prio_sample
inline int prio_sample_call(PrioShape* s, const wh_replay_prio* t, int64_t M, const int64_t* idx_out) {
  if (M > 0 && !idx_out) return WH_EINVAL;
  const int rc = prio_tree(t, s);
  if (rc) return rc;
  return M < 0 ? WH_EINVAL : WH_OK;
}

// ----------------------------------------------------------------------------- SAC TD targets
// wh_sac_td: the sizes first (a, M, NA), then -- for M > 0 only, as everywhere -- the pointers: at
// least one output, the four required inputs, and what an output or option needs beside it.
constexpr int32_t SAC_MAX_AGENTS = 16;

inline int sac_td_call(int64_t M, int32_t NA, const wh_sac_td_args* a) {
  if (!a || M < 0 || NA < 1 || NA > SAC_MAX_AGENTS) return WH_EINVAL;
  if (M == 0) return WH_OK;
  if (!a->y && !a->td_rows && !a->td) return WH_EINVAL;
  if (!a->pi_next || !a->q1t_next || !a->actions || !a->rewards) return WH_EINVAL;
  if ((a->td_rows || a->td || a->q2) && !a->q1) return WH_EINVAL;
  return (a->mask_dones != 0 && !a->dones) ? WH_EINVAL : WH_OK;
}

// wh_sac_td_la: wh_sac_td's rules, then -- for M > 0 -- the pointer alpha is read through.
inline int sac_td_la_call(int64_t M, int32_t NA, const wh_sac_td_args* a, const float* log_alpha) {
  const int rc = sac_td_call(M, NA, a);
  if (rc || M == 0) return rc;
  return log_alpha ? WH_OK : WH_EINVAL;
}

// ----------------------------------------------------------------------------- SAC losses
// wh_sac_loss / wh_sac_loss_query: the sizes first, then -- for M > 0 only -- the pointers.  A
// workgroup (and the host engine's unit of `work`) owns floor(256 / NA) whole samples, like wh_sac_td;
// `work` holds SAC_LOSS_PARTIALS floats per workgroup.
constexpr int32_t SAC_LOSS_PARTIALS = 8;   // sum c1, sum c2, sum f, sum t, live rows, 3 unused (32 bytes)

inline int64_t sac_loss_groups(int64_t M, int32_t NA) {
  const int64_t spw = 256 / NA;
  return (M + spw - 1) / spw;
}

inline int sac_loss_query_call(int64_t M, int32_t NA, int64_t* work_bytes) {
  if (M < 0 || NA < 1 || NA > SAC_MAX_AGENTS) return WH_EINVAL;
  const int64_t groups = sac_loss_groups(M, NA);
  if (work_bytes) *work_bytes = (groups > 0 ? groups : 1) * SAC_LOSS_PARTIALS * (int64_t)sizeof(float);
  return WH_OK;
}

inline int sac_loss_call(int64_t M, int32_t NA, const wh_sac_loss_args* a) {
  if (!a || M < 0 || NA < 1 || NA > SAC_MAX_AGENTS) return WH_EINVAL;
  if (M == 0) return WH_OK;
  if (!a->pi || !a->q1 || !a->y || !a->actions || !a->log_alpha || !a->stats) return WH_EINVAL;
  if (a->dq2 && !a->q2) return WH_EINVAL;
  return (!a->work || ((uintptr_t)a->work & 15u)) ? WH_EINVAL : WH_OK;
}

// ----------------------------------------------------------------------------- Adam
// wh_adam_step: the count of segments, h, segs, then every segment: its count, and for count > 0 its
// four pointers, each 4-byte aligned.
inline int adam_segs(int32_t nseg, const wh_adam_seg* segs) {
  if (nseg > 0 && !segs) return WH_EINVAL;
  for (int32_t s = 0; s < nseg; ++s) {
    const wh_adam_seg& g = segs[s];
    if (g.count < 0) return WH_EINVAL;
    if (g.count == 0) continue;
    if (!g.p || !g.m || !g.v || !g.g) return WH_EINVAL;
    if (((uintptr_t)g.p | (uintptr_t)g.m | (uintptr_t)g.v | (uintptr_t)g.g) & 3u) return WH_EINVAL;
  }
  return WH_OK;
}

inline int adam_call(int32_t nseg, const wh_adam_seg* segs, const wh_adam_hyper* h) {
  if (nseg < 0 || nseg > WH_ADAM_MAX_SEGS || !h) return WH_EINVAL;
  return adam_segs(nseg, segs);
}

// wh_adam_step_clock: the count of segments, the clock and its alignment, then the segments as above.
inline int adam_clock_call(int32_t nseg, const wh_adam_seg* segs, const wh_adam_clock* clock) {
  if (nseg < 0 || nseg > WH_ADAM_MAX_SEGS || !clock || ((uintptr_t)clock & 7u)) return WH_EINVAL;
  return adam_segs(nseg, segs);
}

// ----------------------------------------------------------------------------- MLP training
// wh_mlp_train_query / wh_mlp_train_forward / wh_mlp_backward, in the header's order: the desc, its
// shape, its precision, rows < 0, the pointers, the alignment of `work`, the empty batch, the row limit.
inline bool mlp_train_shape_ok(const wh_mlp_desc* d) {
  const int32_t shapes[3][3] = {{37, 256, 256}, {82, 512, 512}, {145, 1024, 256}};   // Small, Medium, Large
  for (const auto& s : shapes)
    if (d->in_dim == s[0] && d->hidden0 == s[1] && d->hidden1 == s[2]) return d->out_dim == 9;
  return false;
}

inline int mlp_train_desc(const wh_mlp_desc* d, int64_t rows) {
  if (!d) return WH_EINVAL;
  if (!mlp_train_shape_ok(d) || d->precision != WH_MLP_F32) return WH_ENOTSUP;
  return rows < 0 ? WH_EINVAL : WH_OK;
}

inline bool mlp_weights_ok(const wh_mlp_weights* w) { return w && w->w0 && w->b0 && w->w1 && w->b1 && w->w2 && w->b2; }
inline bool mlp_grads_ok(const wh_mlp_grads* g) { return g && g->w0 && g->b0 && g->w1 && g->b1 && g->w2 && g->b2; }

inline int mlp_train_query_call(const wh_mlp_desc* d, int64_t rows) {
  const int rc = mlp_train_desc(d, rows);
  if (rc) return rc;
  return rows > WH_MLP_TRAIN_MAX_ROWS ? WH_EINVAL : WH_OK;
}

// *live = 0: WH_OK with nothing to launch (rows == 0)
inline int mlp_train_forward_call(const wh_mlp_desc* d, const wh_mlp_weights* w, int64_t rows, const float* obs,
                                  const float* h0, const float* h1, const float* logits, bool* live) {
  *live = false;
  const int rc = mlp_train_desc(d, rows);
  if (rc) return rc;
  if (!mlp_weights_ok(w) || !obs || !h0 || !h1 || !logits) return WH_EINVAL;
  if (rows > WH_MLP_TRAIN_MAX_ROWS) return WH_EINVAL;
  *live = rows > 0;
  return WH_OK;
}

// (rows == 0 is live: the six gradients are written, as zeros)
inline int mlp_backward_call(const wh_mlp_desc* d, const wh_mlp_weights* w, int64_t rows, const float* obs,
                             const float* h0, const float* h1, const float* dlogits, const wh_mlp_grads* g,
                             const void* work) {
  const int rc = mlp_train_desc(d, rows);
  if (rc) return rc;
  if (!mlp_weights_ok(w) || !obs || !h0 || !h1 || !dlogits || !mlp_grads_ok(g) || !work) return WH_EINVAL;
  if ((uintptr_t)work % 16 != 0) return WH_EINVAL;
  return rows > WH_MLP_TRAIN_MAX_ROWS ? WH_EINVAL : WH_OK;
}

// wh_mlp_train_forward_multi / wh_mlp_backward_multi, in the header's order: the desc, its shape and
// precision, rows, the count of jobs, every job's own pointers in ascending order (all jobs before any
// pair is looked at), then the buffers two jobs would both write.  Reads jobs[0 .. nnets - 1] only.
inline int mlp_train_multi_call(const wh_mlp_desc* d, int32_t nnets, const wh_mlp_train_job* jobs, int64_t rows,
                                bool backward) {
  if (!d) return WH_EINVAL;
  if (!mlp_train_shape_ok(d) || d->precision != WH_MLP_F32) return WH_ENOTSUP;
  if (rows < 0 || rows > WH_MLP_TRAIN_MAX_ROWS) return WH_EINVAL;
  if (nnets < 0 || nnets > WH_MLP_TRAIN_MAX_NETS || (nnets > 0 && !jobs)) return WH_EINVAL;
  for (int32_t i = 0; i < nnets; ++i) {
    const wh_mlp_train_job& j = jobs[i];
    if (!mlp_weights_ok(&j.w) || !j.obs || !j.h0 || !j.h1) return WH_EINVAL;
    if (!backward && !j.logits) return WH_EINVAL;
    if (backward && (!j.dlogits || !mlp_grads_ok(&j.g) || !j.work || (uintptr_t)j.work % 16 != 0)) return WH_EINVAL;
  }
  for (int32_t i = 1; i < nnets; ++i)
    for (int32_t o = 0; o < i; ++o) {
      const wh_mlp_train_job &a = jobs[o], &b = jobs[i];
      if (!backward && (a.h0 == b.h0 || a.h1 == b.h1 || a.logits == b.logits)) return WH_EINVAL;
      if (backward && (a.work == b.work || a.g.w0 == b.g.w0 || a.g.b0 == b.g.b0 || a.g.w1 == b.g.w1 ||
                       a.g.b1 == b.g.b1 || a.g.w2 == b.g.w2 || a.g.b2 == b.g.b2))
        return WH_EINVAL;
    }
  return WH_OK;
}

// the quantisation rule, one for both engines (plain C++: also device code)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t prio_quantise(float p) {
  const float x = p * 1048576.0f;
  if (!(x >= 1.0f)) return 1u;   // (a NaN fails the comparison)
  if (x >= 2147483648.0f) return WH_PRIO_MAX;
  return (uint32_t)x;
}

}  // namespace wh_abi
