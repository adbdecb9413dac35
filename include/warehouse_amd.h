/*
 * warehouse_amd.h -- C ABI of the MI355X (gfx950) batched warehouse simulator.
 *
 * Drop-in boundary for the hot path of ffahleraz/rllib-warehouse: `Warehouse.reset()` /
 * `Warehouse.step()` (warehouse/core.py:167-442) and the greedy baseline policy
 * (baseline/solvers.py:27-58), run for B independent episodes on one GPU.  Plain pointers and
 * sizes only; every pointer named "device" is HIP device memory, `stream` is a hipStream_t
 * (NULL = the default stream).  The host engine (libwarehouse_host.so, csrc/host_engine.cpp: the
 * same entry points on host cores, for hosts without a GPU) takes host memory for every "device"
 * pointer, ignores `stream`, runs synchronously, and returns WH_ENOTSUP for the device-only entry
 * points (policy network, fragment operand, two-stream and prepared launches, assert mode, the
 * 16-lanes-per-env execution form wh_*_wide).
 * All calls are asynchronous on `stream` except where noted, return
 * WH_OK (0) or a WH_E* code, and never throw.  The reference is Python, so the binding a maintainer
 * adds on the reference side is ctypes; `warehouse/_native.py` is that binding.
 *
 * PACKED STATE (device, struct-of-arrays across the batch, word-plane major):
 *   state[w * B + e] is 32-bit word w of env e, 0 <= w < wh_layout.words_per_env:
 *     w = 0            header : bits 0-15 t (episode time, core.py:165), bits 16-23 n (live agents),
 *                               bit 24 fresh (set by reset: observation availabilities read 0,
 *                               core.py:233)
 *     w = 1            episode counter (bumped by every reset; keys the philox streams)
 *     w = 2 .. 2+NA-1  agent slot i: byte0 x, byte1 dx, byte2 y, byte3 dy (core.py:153-154), where
 *                      (dx, dy) is the cell of the agent's delivery target and 0xFF,0xFF when it
 *                      carries nothing; slots >= n hold 0xFF00FF00 (idle at (0,0))
 *     next P/4 words   pickup point j, byte j%4 of word j/4: (request target + 1, 0 = no request)
 *                      (core.py:158)
 *     next P/4 words   pickup point j: low 8 bits of the step at which its request expires
 *                      (opened at step t0: t0 + W; steps left = (byte - t) mod 256, core.py:159;
 *                      don't-care when the point has no request)
 *   NA = cfg.agent_slots, P = 4 * num_racks^2.
 *
 * RNG MODES.  Every draw the reference takes from numpy's global MT19937 stream can either be
 * INJECTED (explicit arrays below: bit-exact parity with the reference given its draws) or taken
 * from the PHILOX contract: Philox4x32-10 keyed by `seed`, counter (env_offset + e, episode, t,
 * purpose << 24 | block); purposes RESET=1, REGEN=2, POLICY=3, RANDOM=4 (word layout in
 * DESIGN.md §RNG and oracle/philox.py; 5 = the policy network's sampling noise, 6 = replay index
 * draws, 7 = prioritized replay masses, with the counters their entry points state).  Philox trajectories depend only on the global env id,
 * so any sharding of env ids over GPUs reproduces them exactly.
 */
#ifndef WAREHOUSE_AMD_H
#define WAREHOUSE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WH_OK 0
#define WH_EINVAL 22      /* bad pointer / size / value */
#define WH_ENOTSUP 95     /* a layout this build has no kernel for */
#define WH_EHIP 1000      /* + hipError_t: a HIP runtime error */

#define WH_MAX_RACKS 8

/* Variant geometry.  Mirrors the constructor of warehouse/core.py:78-86
 * (the variant table is warehouse/variants.py:25-62). */
typedef struct wh_config {
  int32_t area_dimension;        /* D                          core.py:82 */
  int32_t num_requests;          /* R (always-open requests)   core.py:81 */
  int32_t num_racks;             /* len(pickup_racks_arrangement) */
  int32_t racks[WH_MAX_RACKS];   /* pickup_racks_arrangement   core.py:83 */
  int32_t agent_slots;           /* NA: agent records per env (num_agents, or max_num_agents for
                                    the Train variants, variants.py:65-98); 1 <= NA <= R */
  int32_t episode_duration;      /* T                          core.py:84 */
  int32_t pickup_wait_duration;  /* W (<= 255)                 core.py:85 */
} wh_config;

typedef struct wh_layout {
  int32_t words_per_env;   /* packed state words per env */
  int32_t num_pickups;     /* P  = 4 * num_racks^2        core.py:96 */
  int32_t num_deliveries;  /* Dp = 4 * (D - 4)            core.py:97 */
  int32_t obs_len;         /* 9R + 1 floats per agent row, sorted gym.spaces.Dict key order */
  int32_t kernel_agents;   /* compile-time agent bound of the kernel chosen for this config */
} wh_layout;

/* Validate `cfg` and describe its packed layout.  Host only, synchronous. */
int wh_query(const wh_config* cfg, wh_layout* out);

/* Canonical <-> packed state.  Canonical arrays are int32 device tensors:
 *   pos [B,NA,2], agent_target [B,NA] (-1 idle), pickup_target [B,P] (-1 none),
 *   pickup_timer [B,P] (-1 none), t [B], n [B]; fresh [B] uint8; episode [B] uint32.
 * (the reference's own state arrays, core.py:150-165) */
int wh_pack(const wh_config* cfg, int64_t B, const int32_t* pos, const int32_t* agent_target,
            const int32_t* pickup_target, const int32_t* pickup_timer, const int32_t* t,
            const int32_t* n, const uint8_t* fresh, const uint32_t* episode, uint32_t* state,
            void* stream);
int wh_unpack(const wh_config* cfg, int64_t B, const uint32_t* state, int32_t* pos,
              int32_t* agent_target, int32_t* pickup_target, int32_t* pickup_timer, int32_t* t,
              int32_t* n, uint8_t* fresh, uint32_t* episode, void* stream);

/* Injected reset draws (core.py:191-221): accepted spawn cells, the R opened pickups and their
 * targets in draw order, and (Train variants, variants.py:73-74) the agent count. */
typedef struct wh_reset_draws {
  const int32_t* spawn;    /* [B,NA,2] */
  const int32_t* pickups;  /* [B,R]    distinct pickup indices */
  const int32_t* targets;  /* [B,R]    delivery indices */
  const int32_t* n;        /* [B] or NULL (= NA) */
} wh_reset_draws;

/* Warehouse.reset()  (warehouse/core.py:167-260; Train variants variants.py:69-71).
 * mask [B] uint8 or NULL (all); draws NULL = philox; variable_n != 0 draws n ~ U{1..NA}. */
int wh_reset(const wh_config* cfg, int64_t B, uint32_t* state, const uint8_t* mask,
             const wh_reset_draws* draws, int32_t variable_n, uint64_t seed, int64_t env_offset,
             void* stream);

#define WH_PHASE_ALL 0        /* the whole of core.py:262-442 */
#define WH_PHASE_PRE_REGEN 1  /* everything but regeneration (core.py:267-335, 354-442);
                                 writes n_inactive so a host can draw the reference's
                                 np.random.choice(inactive, k) before WH_PHASE_REGEN */
#define WH_PHASE_REGEN 2      /* regeneration only (core.py:338-351) */

/* Warehouse.step(action_dict)  (warehouse/core.py:262-442).
 *   actions   [B,NA] int32 in 0..8 (MOVES index, core.py:38; the host wraps -9..-1 like Python)
 *   order     [B,OL] int32 or NULL: action-dict iteration order (core.py:279), -1 entries skipped
 *             (rows are -1 padded); agents not listed do not move.  NULL = ascending agent id.
 *             Entry = agent id in bits 0-7, optionally (bits 8-15) that dict entry's own action + 1,
 *             0 = actions[e,id]: a dict naming one agent under several keys ('0', 0, '-n', -n: int(key)
 *             indexes like numpy, core.py:280) moves it once per entry with that entry's action.
 *   order_len OL, the order row length: 0 = NA, else 1 .. 4*NA (a dict may name every agent under
 *             all four of its key forms); anything else is WH_EINVAL.
 *   rewards   [B,NA] float32 (core.py:334-368), dones [B] uint8 (core.py:438); either may be NULL
 *   regen     [B,2R] int32 or NULL (philox): R positions into the ascending list of inactive
 *             pickups (the index np.random.choice(inactive,k) picked), then R delivery targets;
 *             only the first k = R - P + |inactive| of each are read.
 *   n_inactive [B] int32 or NULL: |inactive| before regeneration (core.py:338). */
int wh_step(const wh_config* cfg, int64_t B, uint32_t* state, const int32_t* actions,
            const int32_t* order, int32_t order_len, float* rewards, uint8_t* dones, const int32_t* regen,
            int32_t* n_inactive, int32_t phase, uint64_t seed, int64_t env_offset, void* stream);

/* Per-agent observation rows (core.py:224-260 after reset, 371-432 after a step, including the
 * row-1 quirk of core.py:428), flattened in sorted-key order:
 *   num_agents, other_availabilities, other_delivery_targets, other_positions, requests,
 *   self_availability, self_delivery_target, self_position
 * obs [B,NA,9R+1] float32; rows of slots >= n are zero. */
int wh_observe(const wh_config* cfg, int64_t B, const uint32_t* state, float* obs, void* stream);
/* wh_observe plus (xfrag != NULL) the same rows as the SAC policy network's layer-0 operand, for
 * wh_mlp_forward_x: bf16 in MFMA fragment order, ceil(B*NA/32) tiles of 32 agent rows x KQ =
 * ceil((9R+3)/16) k-steps x 64 lanes x 16 bytes; 16-byte chunk ((tile*KQ + q)*64 + lane) = features
 * 16q + 8(lane>>5) + j, j < 8, of row tile*32 + (lane&31), features 9R+1 and 9R+2 = 1.0, padding 0
 * (rows past B*NA: zero features but the two 1.0 columns).  obs may be NULL.  Every agent count
 * is supported; xfrag must be 16-byte aligned. */
int wh_observe_x(const wh_config* cfg, int64_t B, const uint32_t* state, float* obs, void* xfrag, void* stream);

#define WH_POLICY_EXTERNAL 0  /* the caller's actions (wh_replay_record) */
#define WH_POLICY_GREEDY 1    /* baseline/solvers.py:27-58 with random_action_prob p */
#define WH_POLICY_RANDOM 2    /* uniform over the 9 moves (action_space.sample()) */

/* WarehouseRandomGreedySolver.compute_action (baseline/solvers.py:27-58) evaluated on the state,
 * or uniform random actions: writes actions [B,NA] int32 (slots >= n get 4 = stay). */
int wh_policy(const wh_config* cfg, int64_t B, const uint32_t* state, int32_t policy, float p,
              int32_t* actions, uint64_t seed, int64_t env_offset, void* stream);

/* Episode metrics of scripts/train.py:18-23 (on_episode_end: avg_agent_reward = episode return
 * summed over agents / n, reported overall and per n), accumulated on the device.  Rewards are
 * whole numbers, so returns are kept as integers and every total is exact and order-independent:
 * the mean avg_agent_reward of the episodes with n agents is return_sum[n] / (n * episodes[n]).
 * Bins are indexed by n (arrays of agent_slots + 1); the caller zeroes them (return_min to
 * 0xFFFFFFFF).  `episode_return` is required when any bin pointer is set; others may be NULL.
 * An episode is counted at the step whose done flag is set; continuing a done env without a reset
 * counts it again (the reference has no guard after done either, core.py:438). */
typedef struct wh_episode_stats {
  uint32_t* episode_return;  /* [B]      running return of each env's current episode (read+write) */
  uint64_t* return_sum;      /* [NA + 1] += return of every finished episode, binned by its n */
  uint64_t* episodes;        /* [NA + 1] += finished episodes */
  uint32_t* return_min;      /* [NA + 1] min= episode return */
  uint32_t* return_max;      /* [NA + 1] max= episode return */
} wh_episode_stats;

/* Device-resident rollout: `steps` iterations of {policy, step, auto-reset at t >= T} in one
 * launch (the loop of baseline/run.py:42-62 without the host).  State stays in registers between
 * iterations.  rewards [steps,B,NA] / dones [steps,B] / returns [B] (+= sum of rewards) / stats
 * may each be NULL.  Philox draws only. */
int wh_rollout(const wh_config* cfg, int64_t B, uint32_t* state, int32_t steps, int32_t policy,
               float p, float* rewards, uint8_t* dones, float* returns, const wh_episode_stats* stats,
               int32_t autoreset, int32_t variable_n, uint64_t seed, int64_t env_offset, void* stream);

/* One step of an RLlib-style vectorised sampler (the route scripts/train.py's workload takes:
 * policy actions in, {obs, rewards, dones} out, done episodes restarted): wh_step with philox
 * draws, then (autoreset != 0) a philox reset of every env whose episode ended -- Train variants
 * (variable_n != 0) redraw n there, variants.py:69-71 -- then wh_observe into obs (NULL = skip).
 * With autoreset the obs rows of a done env are the first rows of its next episode.
 *   actions [B,NA] int32 0..8 (others act as 4 = stay)
 *   order   [B,OL] int32 or NULL (OL = order_len as in wh_step): each env's action-dict iteration
 *           order (core.py:279), -1 padded; agents not listed are skipped -- they neither move nor
 *           re-mark their cell (core.py:279-300 only visits the dict's keys).  NULL = every agent,
 *           ascending id.  Entries as wh_step's (bits 8-15: the entry's own action + 1, for repeated
 *           agents).
 *   mask [B] uint8 or NULL: only envs with mask != 0 are stepped (the others keep their state;
 *   their rewards/dones are not written); rewards [B,NA] / dones [B] / obs [B,NA,9R+1] / stats
 *   may be NULL. */
int wh_vector_step(const wh_config* cfg, int64_t B, uint32_t* state, const int32_t* actions,
                   const int32_t* order, int32_t order_len, const uint8_t* mask, float* rewards, uint8_t* dones, float* obs,
                   const wh_episode_stats* stats, int32_t autoreset, int32_t variable_n,
                   uint64_t seed, int64_t env_offset, void* stream);

/* wh_vector_step writing the rows as wh_observe_x's fragment-order operand (xfrag, 16-byte
 * aligned, [ceil(B*NA/32), KQ, 64, 16] bytes, KQ = (9R+1+2+15)/16) instead of f32 rows: the step of
 * the policy route of scripts/rollout.py:72 (network forward on the operand -> env.step -> next
 * operand).  The same transitions and operand bytes as wh_vector_step(obs = NULL) followed by
 * wh_observe_x (which is what it runs). */
int wh_vector_step_x(const wh_config* cfg, int64_t B, uint32_t* state, const int32_t* actions,
                     const int32_t* order, int32_t order_len, const uint8_t* mask, float* rewards, uint8_t* dones, void* xfrag,
                     const wh_episode_stats* stats, int32_t autoreset, int32_t variable_n,
                     uint64_t seed, int64_t env_offset, void* stream);

/* One step of the sampler route with the device policy (the greedy solver of baseline/solvers.py:27-58
 * standing in for the learner's policy, or uniform random actions): policy + step + auto-reset
 * (Train variants redraw n) in one step launch, then the observation rows (wh_observe); the same
 * philox draws and results as wh_policy followed by wh_vector_step(autoreset = 1), one launch
 * fewer.  rewards [B,NA] / dones [B] / obs [B,NA,9R+1] / stats may be NULL. */
int wh_sampler_step(const wh_config* cfg, int64_t B, uint32_t* state, int32_t policy, float p,
                    float* rewards, uint8_t* dones, float* obs, const wh_episode_stats* stats,
                    int32_t variable_n, uint64_t seed, int64_t env_offset, void* stream);

/* `steps` consecutive wh_sampler_step's in ONE launch (a rollout fragment of the sampler route):
 * rewards [steps,B,NA] / dones [steps,B] / obs [steps,B,NA,9R+1] (obs required), step k's outputs at
 * index k; the same draws, transitions and rows as `steps` calls of wh_sampler_step.  In the fused
 * launch the simulation of step k runs while step k-1's rows stream out, the state staying in
 * registers; configurations it does not cover run the steps one call at a time. */
int wh_sampler_rollout(const wh_config* cfg, int64_t B, uint32_t* state, int32_t steps, int32_t policy, float p,
                       float* rewards, uint8_t* dones, float* obs, const wh_episode_stats* stats, int32_t variable_n,
                       uint64_t seed, int64_t env_offset, void* stream);

/* wh_sampler_step's step launch with the state double-buffered and no observation rows: reads
 * state_in, writes the stepped state to state_out (a distinct [words, B] buffer, or state_in itself).
 * With two state buffers, wh_observe of step s (reading its output buffer) can run on another stream
 * while step s + 1 reads the same buffer and writes the other one (warehouse/vector.py
 * SamplerPipeline); the results are those of wh_sampler_step. */
int wh_sampler_step_to(const wh_config* cfg, int64_t B, const uint32_t* state_in, uint32_t* state_out,
                       int32_t policy, float p, float* rewards, uint8_t* dones, const wh_episode_stats* stats,
                       int32_t variable_n, uint64_t seed, int64_t env_offset, void* stream);

/* A second execution form of the step for small batches: one env spread over WH_WIDE_LANES lanes (4 envs
 * per wave, 16 per workgroup; csrc/step_wide.h) instead of one env per lane, so the per-agent and
 * per-pickup phases of a step take O(1) lane steps.  Same packed state, philox contract, outputs and
 * transitions, bit for bit: a wide launch and a lane-per-env launch may alternate on one state buffer.
 * Each entry mirrors the one it is named after (ascending agent order, the whole step: no `order`, no
 * split phases, no state_out, no fused observation rows) with a trailing `lanes`:
 *   lanes == WH_WIDE_LANES  the wide kernel;
 *   lanes == 1              the lane-per-env entry point itself (order = NULL, WH_PHASE_ALL);
 *   anything else           WH_EINVAL.
 * wh_step_wide writes n_inactive (when not NULL) although it runs the whole step.  wh_vector_step_wide
 * is the wide step launch followed by wh_observe (obs may be NULL).  Device only. */
#define WH_WIDE_LANES 16
int wh_step_wide(const wh_config* cfg, int64_t B, uint32_t* state, const int32_t* actions, float* rewards,
                 uint8_t* dones, const int32_t* regen, int32_t* n_inactive, uint64_t seed, int64_t env_offset,
                 int32_t lanes, void* stream);
int wh_rollout_wide(const wh_config* cfg, int64_t B, uint32_t* state, int32_t steps, int32_t policy, float p,
                    float* rewards, uint8_t* dones, float* returns, const wh_episode_stats* stats,
                    int32_t autoreset, int32_t variable_n, uint64_t seed, int64_t env_offset, int32_t lanes,
                    void* stream);
int wh_vector_step_wide(const wh_config* cfg, int64_t B, uint32_t* state, const int32_t* actions,
                        const uint8_t* mask, float* rewards, uint8_t* dones, float* obs,
                        const wh_episode_stats* stats, int32_t autoreset, int32_t variable_n, uint64_t seed,
                        int64_t env_offset, int32_t lanes, void* stream);

/* A prepared wh_rollout: the same arguments resolved once (config validated, kernel and tables
 * chosen) into an opaque handle, so a loop that launches the same rollout repeatedly pays one
 * cheap call per launch (wh_launch_run enqueues exactly what wh_rollout would).  The buffers must
 * stay valid while the handle is used; free it with wh_launch_free. */
typedef struct wh_launch wh_launch;
int wh_rollout_prepare(const wh_config* cfg, int64_t B, uint32_t* state, int32_t steps, int32_t policy,
                       float p, float* rewards, uint8_t* dones, float* returns, const wh_episode_stats* stats,
                       int32_t autoreset, int32_t variable_n, uint64_t seed, int64_t env_offset, void* stream,
                       wh_launch** out);
int wh_launch_run(const wh_launch* launch);
/* wh_launch_run with HIP events (hipEvent_t, created by the caller with timing enabled) attached to
 * the kernel dispatch itself (hipExtLaunchKernel): start/stop are stamped when the kernel starts and
 * ends, so their span is the kernel's duration and no separate marker packets sit in the stream.
 * Either event may be NULL (e.g. start on the first of several launches, stop on the last). */
int wh_launch_run_timed(const wh_launch* launch, void* start_event, void* stop_event);
/* Frees a handle of wh_rollout_prepare.  Handles are tracked: run / run_timed / free of a pointer that
 * is not a live handle (never prepared, or already freed) return WH_EINVAL and touch nothing, so a
 * double free is refused instead of corrupting the heap -- as long as no later wh_rollout_prepare
 * has been handed the same address: a freed handle whose address the allocator reuses is live again
 * (it names the new launch), so a stale pointer must not be used after a further prepare.  NULL is
 * a no-op (WH_OK).  A prepare with B = 0 needs no device and no tables: its handle launches nothing. */
int wh_launch_free(wh_launch* launch);

/* SAC policy network forward (the policy_model of scripts/experiments/warehouse-{small,medium,large}-sac: a
 * ReLU MLP, hidden_layer_sizes [256,256] Small / [512,512] Medium / [1024,256] Large, 9 action
 * logits), i.e. trainer.compute_action(obs) of scripts/rollout.py:72 for every agent row of a
 * batch.  precision WH_MLP_BF16: bf16 MFMA with f32 accumulation, activations rounded to bf16
 * between layers (fast); WH_MLP_F32: exact f32 (v_mfma_f32_32x32x2_f32, an fmaf chain per output:
 * logits equal a float32 reference up to summation order), like the reference's TF fp32 policy.
 * Supported: in_dim = 9R+1 of a variant with its hidden sizes, out_dim = 9 (else WH_ENOTSUP).
 * Blobs are precision-specific: pack and forward with the same desc. */
#define WH_MLP_BF16 0
#define WH_MLP_F32 1
typedef struct wh_mlp_desc {
  int32_t in_dim, hidden0, hidden1, out_dim;
  int32_t precision; /* WH_MLP_BF16 or WH_MLP_F32 */
} wh_mlp_desc;

/* Size of the packed weight blob (device bytes).  Host only. */
int wh_mlp_query(const wh_mlp_desc* d, int64_t* packed_bytes);

/* Pack host f32 weights in torch nn.Linear layout (w0 [hidden0, in_dim], b0 [hidden0],
 * w1 [hidden1, hidden0], b1 [hidden1], w2 [out_dim, hidden1], b2 [out_dim]) into the device blob
 * `packed` (wh_mlp_query bytes, 16-byte aligned).  Synchronous. */
int wh_mlp_pack(const wh_mlp_desc* d, const float* w0, const float* b0, const float* w1,
                const float* b1, const float* w2, const float* b2, void* packed);

/* wh_mlp_pack with w0..b2 in DEVICE memory (same layouts), as kernels on `stream`: no host copy of the
 * weights, no synchronisation.  The blob is byte-for-byte the one wh_mlp_pack makes from the same values
 * (both run the same index maps and the same integer round-to-nearest-even), so a learner that keeps
 * its parameters on the card refreshes a rollout network, or a Q network, without leaving the stream.
 * One launch.  The first call for a shape and device uploads that shape's operand table (a few KB):
 * that call allocates and copies synchronously and must not happen inside a stream capture; every
 * later call for the shape on that device only enqueues.  `packed`: wh_mlp_query bytes, 16-byte
 * aligned (else WH_EINVAL).  d == NULL or any pointer NULL: WH_EINVAL; an unknown shape: WH_ENOTSUP.
 * Device only. */
int wh_mlp_pack_device(const wh_mlp_desc* d, const float* w0, const float* b0, const float* w1,
                       const float* b1, const float* w2, const float* b2, void* packed, void* stream);

/* obs [rows, in_dim] f32 -> logits [rows, 9] f32 and/or actions [rows] int32 (either may be NULL,
 * not both).  explore = 0: argmax, first maximum wins; explore = 1: Gumbel-max sample of
 * Categorical(logits): the first maximum of logit[o] - log(-log u[o]), the noise from the philox
 * contract, purpose 5: counter (row & 0xFFFFFFFF, row >> 32, step, 5 << 24 | block) keyed by seed
 * (low word, high word), row the row's index in this launch, blocks 0-2; action o takes word o of the
 * twelve (9-11 unused) as u = (float(w >> 8) + 0.5f) * 2^-24 in f32.  u lies in (0, 1]: the largest
 * 24-bit draw rounds to exactly 1, whose noise is +inf, and that action is taken. */
int wh_mlp_forward(const wh_mlp_desc* d, const void* packed, int64_t rows, const float* obs,
                   float* logits, int32_t* actions, int32_t explore, uint64_t seed, uint32_t step,
                   void* stream);
/* wh_mlp_forward with the observation rows given as wh_observe_x's fragment-order operand (bf16
 * precision only; the same logits as wh_mlp_forward on the f32 rows, which it rounds to bf16
 * exactly so): one coalesced 16-byte load per k-step and lane instead of strided f32 rows. */
int wh_mlp_forward_x(const wh_mlp_desc* d, const void* packed, int64_t rows, const void* xfrag,
                     float* logits, int32_t* actions, int32_t explore, uint64_t seed, uint32_t step,
                     void* stream);

/* Several forwards of ONE network shape in one launch: up to WH_MLP_MAX_JOBS (network, input, output)
 * jobs that share `d` run side by side, the launch's workgroups shared out among them by their row
 * counts (csrc/mlp_grid.h).  A forward of a few hundred rows fills a few CUs; a SAC learner's three or
 * five such forwards (policy, target Qs, Qs) then cost about one instead of running one after the other.
 * For every job, `logits` and `actions` hold byte for byte what wh_mlp_forward (obs) or wh_mlp_forward_x
 * (xfrag) writes for the same arguments.  One launch on `stream`; no host sync, no allocation.  A bf16
 * job reads either `obs` or `xfrag`, each job as it likes.
 * Checked in this order before anything is launched (a refused call launches and writes nothing):
 * d == NULL WH_EINVAL; an unknown shape WH_ENOTSUP; njobs < 0 or > WH_MLP_MAX_JOBS, or njobs > 0 with
 * jobs == NULL, WH_EINVAL; then per job the rules of wh_mlp_forward: rows < 0 WH_EINVAL, rows == 0 skips
 * the job (its other fields are not looked at), packed NULL / no input / no output / both inputs
 * WH_EINVAL, xfrag with WH_MLP_F32 or not 16-byte aligned WH_ENOTSUP; two live jobs with the same
 * non-NULL logits or the same non-NULL actions WH_EINVAL; an f32 launch of more than 2^31 - 1 blocks
 * (128 rows each) WH_EINVAL.  No live job: WH_OK, nothing launched.  Device only. */
#define WH_MLP_MAX_JOBS 8
typedef struct wh_mlp_job {
  const void* packed;  /* this job's blob (wh_mlp_pack / wh_mlp_pack_device) */
  int64_t rows;
  const float* obs;    /* f32 rows, or NULL */
  const void* xfrag;   /* fragment-order operand, or NULL (bf16 only, 16-byte aligned) */
  float* logits;       /* [rows, 9] or NULL */
  int32_t* actions;    /* [rows] or NULL */
  int32_t explore;
  uint32_t step;
  uint64_t seed;
} wh_mlp_job;
int wh_mlp_forward_multi(const wh_mlp_desc* d, int32_t njobs, const wh_mlp_job* jobs, void* stream);

/* MLP TRAINING: the same three-layer ReLU network's training forward and backward in exact f32
 * (csrc/mlp_train.h), for a learner that keeps its master weights on the card.  Both read the f32
 * parameters in torch nn.Linear layout (w0 [hidden0, in_dim], b0 [hidden0], w1 [hidden1, hidden0],
 * b1 [hidden1], w2 [9, hidden1], b2 [9]) straight from device memory: no blob.  Device only.
 *
 * wh_mlp_train_forward, all row-major f32, every dot product an f32 fma chain (v_mfma_f32_32x32x2_f32):
 *   h0 [rows, hidden0] = max(W0 x + b0, 0),  h1 [rows, hidden1] = max(W1 h0 + b1, 0),
 *   logits [rows, 9] = W2 h1 + b2.
 * The values equal a float32 reference up to summation order.  The bias is added after the sum here and
 * the k order differs from wh_mlp_forward's, so on real-valued weights the logits need NOT be bit-equal
 * to wh_mlp_forward's WH_MLP_F32 logits (on integer-valued networks whose sums are exact, they are).
 *
 * wh_mlp_backward, with dZ = dlogits [rows, 9] and h0 / h1 as the forward wrote them:
 *   gW2 = dZ^T h1            gb2 = sum_r dZ       dH1 = (dZ W2)  . [h1 > 0]
 *   gW1 = dH1^T h0           gb1 = sum_r dH1      dH0 = (dH1 W1) . [h0 > 0]
 *   gW0 = dH0^T x            gb0 = sum_r dH0
 * The mask is h > 0: a unit whose pre-activation is exactly 0 passes no gradient (torch's relu backward).
 * The six gradients, in the parameters' layouts, are OVERWRITTEN, not accumulated (torch accumulates
 * .grad itself); no gradient w.r.t. obs is produced.  No floating-point atomics: every gradient element
 * is summed in an order fixed by the shape and `rows` alone, so two calls on the same inputs agree bit
 * for bit.  `work` is scratch (dH1, dH0 and, above 512 rows, the partial weight gradients of up to 16
 * row slices, which a second pass adds in slice order); its layout is the kernels' own, its size
 * wh_mlp_train_query's `work_bytes` (never 0), and it is 16-byte aligned.  Neither entry point
 * allocates or synchronises: both only enqueue on `stream` (three launches forward; three backward,
 * four above 512 rows).
 *
 * Checked in this order before anything is launched (a refused call launches and writes nothing):
 * d == NULL WH_EINVAL; a shape that is no variant's, or out_dim != 9, WH_ENOTSUP; precision other than
 * WH_MLP_F32 WH_ENOTSUP (the backward takes f32 operands only); rows < 0 WH_EINVAL; NULL among w and
 * its six pointers, obs, h0, h1, logits (forward) or dlogits (backward), g and its six pointers, work
 * WH_EINVAL; work not 16-byte aligned WH_EINVAL; rows > WH_MLP_TRAIN_MAX_ROWS, the largest the launch
 * geometry is stated for, WH_EINVAL.  rows == 0 is WH_OK: the forward launches nothing, the backward
 * writes zeros to all six gradients.  wh_mlp_train_query applies the rules of d and rows; work_bytes
 * may be NULL. */
#define WH_MLP_TRAIN_MAX_ROWS 16777216 /* 2^24 */
typedef struct wh_mlp_weights { const float *w0, *b0, *w1, *b1, *w2, *b2; } wh_mlp_weights; /* device, nn.Linear layout */
typedef struct wh_mlp_grads { float *w0, *b0, *w1, *b1, *w2, *b2; } wh_mlp_grads;           /* same shapes */
int wh_mlp_train_query(const wh_mlp_desc* d, int64_t rows, int64_t* work_bytes);
int wh_mlp_train_forward(const wh_mlp_desc* d, const wh_mlp_weights* w, int64_t rows, const float* obs,
                         float* h0, float* h1, float* logits, void* stream);
int wh_mlp_backward(const wh_mlp_desc* d, const wh_mlp_weights* w, int64_t rows, const float* obs,
                    const float* h0, const float* h1, const float* dlogits, const wh_mlp_grads* g,
                    void* work, void* stream);

/* The training passes of several networks of ONE shape in one launch per product: up to
 * WH_MLP_TRAIN_MAX_NETS jobs that share `d` and `rows` (one tile geometry, one slice count and one block
 * count per product; jobs may share one obs) run side by side, each launch's workgroups being network
 * 0's, then network 1's, ...  A SAC learner's policy, Q1 and Q2 passes at a few hundred rows are bound
 * by dispatch and by the depth of their MFMA chains, not by bytes: three networks then take three
 * launches forward (one per layer) and three backward (four above 512 rows, the last one adding the
 * partial weight gradients of all networks) instead of nine and nine (twelve).
 * For every job, h0, h1 and logits hold byte for byte what wh_mlp_train_forward writes for that job's
 * arguments and the six gradients byte for byte what wh_mlp_backward writes: a workgroup runs the tile
 * of the single-network launch on the same arguments.  `work` is wh_mlp_backward's (wh_mlp_train_query
 * bytes, 16-byte aligned), one per job.  No allocation, no synchronisation, no atomics.
 * Checked in this order before anything is launched (a refused call launches and writes nothing):
 * d == NULL WH_EINVAL; a shape that is no variant's, out_dim != 9 or a precision other than WH_MLP_F32
 * WH_ENOTSUP; rows < 0 or rows > WH_MLP_TRAIN_MAX_ROWS WH_EINVAL; nnets < 0, nnets >
 * WH_MLP_TRAIN_MAX_NETS, or nnets > 0 with jobs == NULL, WH_EINVAL; then per job in ascending order the
 * pointer rules of the single call -- forward: NULL among w's six pointers, obs, h0, h1, logits;
 * backward: NULL among w's six pointers, obs, h0, h1, dlogits, g's six pointers, work, or work not
 * 16-byte aligned -- WH_EINVAL; then two jobs with the same h0, the same h1 or the same logits
 * (forward), or with the same work or the same pointer in the same field of g (backward), WH_EINVAL.
 * nnets == 0 is WH_OK with nothing launched.  rows == 0 is WH_OK: the forward launches nothing, the
 * backward writes zeros to every job's six gradients.  Device only. */
#define WH_MLP_TRAIN_MAX_NETS 4
typedef struct wh_mlp_train_job {
  wh_mlp_weights w;        /* this network's parameters (device, nn.Linear layout) */
  const float* obs;        /* [rows, in_dim]; jobs may share one obs */
  float *h0, *h1, *logits; /* forward writes all three; backward reads h0, h1 (logits unused there) */
  const float* dlogits;    /* backward only */
  wh_mlp_grads g;          /* backward only */
  void* work;              /* backward only: wh_mlp_train_query(d, rows) bytes, 16-byte aligned, one per job */
} wh_mlp_train_job;
int wh_mlp_train_forward_multi(const wh_mlp_desc* d, int32_t nnets, const wh_mlp_train_job* jobs,
                               int64_t rows, void* stream);
int wh_mlp_backward_multi(const wh_mlp_desc* d, int32_t nnets, const wh_mlp_train_job* jobs,
                          int64_t rows, void* stream);

/* REPLAY RING: off-policy transitions kept as packed states instead of observation rows (every row
 * is a function of the packed state: 265 bytes per Medium-8 transition against 5,289 as f32 rows).
 * A ring holds `capacity` slots; a slot is one time step of all B envs.  The buffers are device
 * memory (host memory for the host engine) owned by the caller, sized exactly as stated; the layout
 * is the same for both engines, so a ring moves between them with a plain copy.  Records are
 * env-major -- states[((slot * 2 + side) * B + e) * words_per_env + w] is word w of env e -- so a
 * sampled transition reads one contiguous record per side. */
typedef struct wh_replay_ring {
  uint32_t* states;   /* [capacity, 2, B, words_per_env]  env-major records; side 0 = the state the
                         actions were chosen from, side 1 = the state after the step and BEFORE any reset */
  uint8_t*  actions;  /* [capacity, B, NA]  0..8 */
  float*    rewards;  /* [capacity, B, NA] */
  uint8_t*  dones;    /* [capacity, B] */
  int64_t   capacity; /* slots (time steps), >= 1 */
} wh_replay_ring;

/* Record one half of slot `slot` (0 <= slot < capacity) from the live [words, B] state, one launch:
 *   stage 0  side 0 of the slot <- state; ring actions <- actions (int32 [B,NA]; values outside 0..8
 *            are kept as 4 = stay, what the step does with them)
 *   stage 1  side 1 of the slot <- state; ring rewards / dones <- rewards (f32 [B,NA]) / dones (u8 [B])
 * The sequence of one recorded step is put(0), a step WITHOUT auto-reset, put(1), then the reset of
 * the done envs: side 1 of a done env is its terminal state (the reference trains with
 * no_done_at_end, so the bootstrap reads the terminal observation), and the next slot's side 0 the
 * fresh state.  The pointers a stage does not read may be NULL. */
int wh_replay_put(const wh_config* cfg, int64_t B, const wh_replay_ring* ring, int64_t slot, int32_t stage,
                  const uint32_t* state, const int32_t* actions, const float* rewards, const uint8_t* dones,
                  void* stream);

/* `steps` recorded steps in one launch, step k into slot (slot + k) % capacity: the same ring bytes,
 * live state, rewards, dones, episode metrics and philox draws as, `steps` times,
 *   [wh_policy ->] wh_replay_put(stage 0) -> wh_vector_step(autoreset = 0, obs = NULL) ->
 *   wh_replay_put(stage 1) -> wh_reset(mask = that step's dones, philox draws, variable_n)
 * followed by wh_observe / wh_observe_x of the final state into obs / xfrag (either or both may be
 * NULL; xfrag 16-byte aligned; a second launch).  policy = WH_POLICY_EXTERNAL steps with `actions`
 * (int32 [B,NA]; steps <= 1), WH_POLICY_GREEDY / WH_POLICY_RANDOM with the device policy and
 * random_action_prob p, whose actions are recorded as wh_policy reports them.  rewards [steps,B,NA]
 * and dones [steps,B] are optional live copies of what the ring receives; `stats` as in wh_rollout.
 * WH_EINVAL: ring NULL or capacity < 1, slot outside [0, capacity), steps < 0 or > capacity, policy
 * not 0 / 1 / 2, policy 0 with steps > 1, p outside [0, 1], bins without episode_return, xfrag
 * misaligned; for B > 0 and steps > 0 a NULL ring array, or policy 0 without actions.  B = 0 or
 * steps = 0 launch nothing.  The host engine returns WH_ENOTSUP when xfrag is given. */
int wh_replay_record(const wh_config* cfg, int64_t B, uint32_t* state, const wh_replay_ring* ring, int64_t slot,
                     int32_t steps, int32_t policy, float p, const int32_t* actions,
                     float* rewards, uint8_t* dones, float* obs, void* xfrag,
                     const wh_episode_stats* stats, int32_t variable_n, uint64_t seed, int64_t env_offset, void* stream);

/* Outputs of wh_replay_gather for M samples; any may be NULL, not all.  obs / next_obs are the rows
 * of wh_observe on side 0 / side 1, xfrag / next_xfrag wh_observe_x's operand for a batch of M envs
 * (device only, 16-byte aligned), state / next_state plane-major packed states [words, M] (usable by
 * every entry that takes a state of M envs). */
typedef struct wh_replay_batch {
  float*    obs;         /* [M, NA, 9R+1] */
  float*    next_obs;    /* [M, NA, 9R+1] */
  void*     xfrag;       /* [ceil(M*NA/32), KQ, 64, 16] bytes */
  void*     next_xfrag;
  uint32_t* state;       /* [words, M] */
  uint32_t* next_state;  /* [words, M] */
  int32_t*  actions;     /* [M, NA] */
  float*    rewards;     /* [M, NA] */
  uint8_t*  dones;       /* [M]  as recorded */
  int32_t*  n;           /* [M]  live agents of side 0 (rows >= n are zero); -1 = invalid index */
  int64_t*  idx_out;     /* [M]  the indices used */
} wh_replay_batch;

/* Gather M transitions of the first `filled` slots (1 <= filled <= capacity) into learner inputs, one
 * launch.  idx [M] int64, each slot * B + env, duplicates and any order allowed; idx = NULL draws
 * them from the philox contract, purpose 6: counter (m, draw & 0xFFFFFFFF, draw >> 32, 6 << 24) keyed
 * by seed, slot = uniform_int(filled, word 0), env = uniform_int(B, word 1).  An index outside
 * [0, filled * B) reads nothing: n[m] = -1 and every other output of sample m is zero (fragment
 * rows keep their two 1.0 columns).  obs / next_obs are written as float4 when NA * (9R+1) is a
 * multiple of 4 and must then be 16-byte aligned.  M = 0 or B = 0 launch nothing.  The host engine
 * returns WH_ENOTSUP when a fragment output is requested. */
int wh_replay_gather(const wh_config* cfg, int64_t B, const wh_replay_ring* ring, int64_t filled, int64_t M,
                     const int64_t* idx, uint64_t seed, uint64_t draw, const wh_replay_batch* batch, void* stream);

/* REPLAY PRIORITIES: a sum tree over the ring's entries for prioritized sampling, in integer
 * arithmetic only, so both engines (and a numpy model) agree bit for bit and no result depends on
 * the order atomics arrive in.  The layout is the same for both engines: a tree moves between them
 * with a plain copy, like the ring.
 *   Index space  leaf i is ring entry i = slot * B + env (the index wh_replay_gather takes);
 *                count = capacity * B leaves, 1 <= count <= 2^31.
 *   Leaves       uint32 fixed-point priorities q, WH_PRIO_ONE = priority 1.0.  A stored q lies in
 *                [1, 2^31 - 1]; 0 = no transition here, never sampled.
 *   Quantising   a priority p (f32, already raised to alpha), x = p * 1048576.0f:
 *                NaN or !(x >= 1) -> q = 1;  x >= 2147483648 -> q = 0x7FFFFFFF;  else q = (uint32_t)x
 *                (the same in every denormal mode: whatever a flush could change is below 1).
 *   Shape        radix 16.  Level 0 is the leaves, padded with zeros to a multiple of 16; level
 *                k >= 1 has n_k = ceil(n_{k-1} / 16) uint64 sums (entry j = the sum of entries
 *                16 j .. 16 j + 15 of level k - 1), padded with zeros to a multiple of 16.  `node`
 *                holds levels 1, 2, ... one after the other; the level with n_k == 1 is the root,
 *                the total (count <= 16: one level above the leaves).  The 16 children of an
 *                entry are 128 bytes, one cache line.  Sums stay below 2^62, so signed deltas
 *                applied as wrapping 64-bit adds are exact.
 * An all-zero tree with *max_q = WH_PRIO_ONE is the empty tree.  The buffers are the caller's, of
 * the sizes wh_replay_prio_query states. */
#define WH_PRIO_ONE (1u << 20)
#define WH_PRIO_MAX 0x7FFFFFFFu
#define WH_PRIO_MAX_COUNT ((int64_t)1 << 31)

typedef struct wh_replay_prio {
  uint32_t* leaf;    /* [leaf_words] */
  uint64_t* node;    /* [node_words]  levels 1 .. levels, bottom-up */
  uint32_t* max_q;   /* [1]  the largest q an update has written (a fresh entry's priority) */
  int64_t   count;   /* leaves: capacity * B */
} wh_replay_prio;

/* Sizes of a tree of `count` leaves: leaf_words uint32, node_words uint64, `levels` levels above
 * the leaves (any output may be NULL).  WH_EINVAL unless 1 <= count <= 2^31. */
int wh_replay_prio_query(int64_t count, int64_t* leaf_words, int64_t* node_words, int32_t* levels);

/* Set leaves [first, first + n) and update their ancestors, one launch:
 *   mode 0  every leaf becomes q (0 <= q <= 2^31 - 1; q = 0 clears the range)
 *   mode 1  every leaf becomes the tree's current *max_q, read on the device (no host sync): what a
 *           recorder does with a fresh slot (RLlib gives new items the maximum priority); q ignored
 * *max_q is left as it is.  n = 0 launches nothing. */
int wh_replay_prio_fill(const wh_replay_prio* tree, int64_t first, int64_t n, int32_t mode, uint32_t q,
                        void* stream);

/* Leaf idx[m] <- quantise(p[m]) for m < M (idx [M] int64, p [M] f32), ancestors updated, *max_q <-
 * the maximum of itself and every q written.  An index outside [0, count) is ignored.  Duplicate
 * indices: the largest q wins, so the result does not depend on execution order.  Two launches on
 * `stream` (clear the touched leaves; raise them to their q).  M = 0 launches nothing. */
int wh_replay_prio_update(const wh_replay_prio* tree, int64_t M, const int64_t* idx, const float* p,
                          void* stream);

/* Draw M leaves with probability q / total, one launch.  Sample m takes r = u[m] (u [M] uint64,
 * injected draws) or, u = NULL, r = w0 << 32 | w1 of the philox contract, purpose 7: counter
 * (m, draw & 0xFFFFFFFF, draw >> 32, 7 << 24) keyed by seed.  mass = (r * total) >> 64; the descent
 * takes in every node the first child whose inclusive prefix sum exceeds the mass left, and
 * subtracts that child's exclusive prefix.  idx_out [M] int64: the leaf reached; q_out [M] (or
 * NULL): its q; total_out [1] (or NULL): the root as this launch read it, so weights can be
 * computed later without racing an update.  An empty tree (total == 0) gives idx_out = -1 and
 * q_out = 0, which wh_replay_gather turns into n = -1 and a zero sample.  M = 0 launches nothing. */
int wh_replay_prio_sample(const wh_replay_prio* tree, int64_t M, const uint64_t* u, uint64_t seed, uint64_t draw,
                          int64_t* idx_out, uint32_t* q_out, uint64_t* total_out, void* stream);

/* SAC TD TARGETS: RLlib's discrete SAC (sac_tf_policy, discrete branch) from logits, one launch.  The
 * Q_model of the experiment YAMLs has the policy_model's shape, so the five [rows, 9] arrays below
 * are what wh_mlp_forward / wh_mlp_forward_x write for the policy, the two target Q networks (on the
 * next-side operand) and the two Q networks (on the obs-side operand).  For row r = m * NA + i, all
 * in f32, sums over o = 0..8 in ascending order:
 *   lse   = zmax + log(sum_o exp(pi_next[r,o] - zmax)),  zmax = max_o pi_next[r,o]
 *   logp  = pi_next[r,o] - lse ;  p = exp(logp)
 *   v     = sum_o p[o] * (min(q1t_next[r,o], q2t_next[r,o]) - alpha * logp[o])     (q2t NULL: q1t alone)
 *   y     = rewards[m,i] + discount * ((mask_dones && dones[m]) ? 0 : v)
 *   a     = actions[m,i] if in 0..8 else 4          (the ring's rule for stray actions)
 *   td_r  = (|q1[r,a] - y| + |q2[r,a] - y|) / 2     (q2 NULL: |q1[r,a] - y|)
 *   td[m] = (sum_{i < n[m]} td_r[m,i]) / n[m]       (n NULL: NA;  n[m] <= 0: 0;  n[m] > NA: as NA)
 * Rows i >= n[m], and every row of a sample with n[m] = -1 (wh_replay_gather's invalid index), write
 * y = 0 and td_rows = 0.  td[m] is ONE priority per ring entry (an env-step, what
 * wh_replay_prio_update takes): the mean of the TD errors of that entry's live agent rows.
 * `discount` is gamma ** n_step, computed by the caller; mask_dones = 0 is what the YAMLs train with
 * (no_done_at_end: true).  td[m] is summed inside one workgroup in ascending row order, without
 * atomics: the result is deterministic.  Inputs are assumed finite; non-finite values propagate as
 * IEEE arithmetic gives and are not part of the contract.
 * WH_EINVAL: a == NULL, M < 0, NA outside 1 .. 16; and for M > 0: all three outputs NULL; pi_next,
 * q1t_next, actions or rewards NULL; td_rows, td or q2 set without q1; mask_dones != 0 with dones
 * NULL.  M = 0 launches nothing (WH_OK, no pointer looked at).  Both engines implement it. */
typedef struct wh_sac_td_args {
  const float *pi_next, *q1t_next, *q2t_next;   /* [M*NA, 9]; q2t_next may be NULL */
  const float *q1, *q2;                         /* [M*NA, 9]; both NULL = targets only; q2 alone NULL = no twin */
  const int32_t* actions;  const float* rewards;  /* [M, NA] */
  const uint8_t* dones;    const int32_t* n;      /* [M]; either may be NULL */
  float alpha, discount;   int32_t mask_dones;
  float *y, *td_rows;      /* [M, NA] out; may be NULL */
  float* td;               /* [M] out; may be NULL */
} wh_sac_td_args;
int wh_sac_td(int64_t M, int32_t NA, const wh_sac_td_args* a, void* stream);
/* wh_sac_td with alpha read where the arithmetic runs: alpha = expf(log_alpha[0]), a->alpha is
 * ignored; everything else is wh_sac_td's.  This is how wh_sac_loss forms its alpha, so the target and
 * the losses of one update use the same value, and a learner needs no host read (nor a stream
 * capture a frozen value).  log_alpha: [1] f32, device memory (host memory on the host engine).
 * WH_EINVAL: wh_sac_td's, and for M > 0 log_alpha == NULL.  M = 0 launches nothing.  Both engines
 * implement it; expf is each engine's own, as in SAC LOSSES (expf(0) = 1 on both). */
int wh_sac_td_la(int64_t M, int32_t NA, const wh_sac_td_args* a, const float* log_alpha, void* stream);

/* SAC LOSSES: the critic, actor and alpha losses of RLlib's discrete SAC (sac_tf_policy, discrete
 * branch) and d(loss)/d(logits), from the learner's own logits at `obs` (what wh_mlp_train_forward
 * writes for the policy and the two Q networks) and the target y of wh_sac_td, which is a constant
 * here.  For a live row r = m * NA + i, all in f32, sums over o = 0..8 in ascending order, no fused
 * multiply-adds:
 *   lse, logp[o], p[o] of pi[r] as in SAC TD TARGETS;  alpha = exp(log_alpha[0]);  w = weights[m]
 *   a         = actions[m,i] if in 0..8 else 4
 *   qm[o]     = min(q1[r,o], q2[r,o])                        (q2 NULL: q1 alone)
 *   g[o]      = alpha * logp[o] - qm[o] ;  f = sum_o p[o] * g[o]               the actor row
 *   dpi[r,j]  = (scale * p[j]) * (g[j] - f)
 *   e_k       = qk[r,a] - y[r] ;  c_k = ((0.5 * w) * e_k) * e_k                the critic rows, k = 1, 2
 *   dqk[r,o]  = (o == a) ? (scale * w) * e_k : 0
 *   t         = sum_o p[o] * (logp[o] + target_entropy)                        the alpha row
 * (d f / d pi[j] also holds alpha p[j] (1 - sum_o p[o]), which is 0 in exact arithmetic and is dropped.)
 * The actor row is policy_t (alpha log_pis_t - stop_gradient(q_t)), the critic rows 0.5 MSE against y
 * with the sampler's importance weights on them, the alpha row stop_gradient(policy_t) (-log_alpha
 * stop_gradient(log_pis_t + target_entropy)).  The Huber critic loss of later RLlib versions is not
 * built.  Rows i >= n[m] (n as in SAC TD TARGETS: NULL = NA, n[m] <= 0 = none) are dead: they write
 * exact zeros to all three gradient arrays and add nothing to any sum.
 *   stats[0] = scale * sum c_1      stats[1] = scale * sum c_2 (0 without q2)     stats[2] = scale * sum f
 *   T = scale * sum t               stats[3] = (-log_alpha[0]) * T, the alpha loss
 *   stats[4] = -T = d(alpha loss) / d(log_alpha)           stats[5] = the number of live rows, as f32
 * `scale` is the caller's normaliser (a mean over all rows: 1 / (M * NA)); it is taken by value so that
 * no pass over n has to count the live rows first, and stats[5] lets a caller renormalise.  log_alpha
 * is read on the device: the call needs no host sync.  No atomics: every workgroup reduces its rows in
 * a fixed order into `work`, and a second launch of one workgroup adds the workgroups' partial sums in a
 * fixed order, so the result is a function of the inputs alone (at most 256 + workgroups additions
 * deep; a batch of one workgroup is a single launch).  The host engine adds in ascending row order.
 * stats[5] is exact up to 2^24 live rows.  `work` is scratch of wh_sac_loss_query's work_bytes (never
 * 0), 16-byte aligned.  Neither entry point allocates or synchronises.  Inputs are assumed finite.
 * WH_EINVAL: a == NULL, M < 0, NA outside 1 .. 16; and for M > 0: pi, q1, y, actions, log_alpha or
 * stats NULL; dq2 set without q2; work NULL or not 16-byte aligned.  M = 0 launches nothing (WH_OK, no
 * pointer looked at, stats untouched).  wh_sac_loss_query applies the rules of M and NA; work_bytes may
 * be NULL.  Both engines implement both. */
typedef struct wh_sac_loss_args {
  const float *pi, *q1, *q2;        /* [M*NA, 9]; q2 may be NULL (no twin) */
  const float* y;                   /* [M, NA] */
  const int32_t* actions;           /* [M, NA] */
  const int32_t* n;                 /* [M] or NULL */
  const float* weights;             /* [M] or NULL (= 1) */
  const float* log_alpha;           /* [1], device memory */
  float target_entropy, scale;
  float *dpi, *dq1, *dq2;           /* [M*NA, 9] out; any may be NULL */
  float* stats;                     /* [6] out */
  void* work;
} wh_sac_loss_args;
int wh_sac_loss_query(int64_t M, int32_t NA, int64_t* work_bytes);
int wh_sac_loss(int64_t M, int32_t NA, const wh_sac_loss_args* a, void* stream);

/* ADAM: one torch.optim.Adam step (no amsgrad, no weight decay, not maximize) over up to
 * WH_ADAM_MAX_SEGS tensors in one launch.  `segs` is a host array that travels in the kernel
 * argument: no table upload, no allocation, no sync.  The caller keeps the step count t and computes
 * the hyper-parameters in double, rounding each once to f32.  Per element, in f32, in this order, no
 * fused multiply-adds, sqrt and divide correctly rounded on both engines:
 *   m' = beta1 * m + omb1 * g ;  v' = beta2 * v + (omb2 * g) * g
 *   p' = p - step_size * (m' / (sqrt(v') / sqrt_bc2 + eps))
 * so the two engines agree bit for bit.  p, m, v are updated in place.  Every pointer is 4-byte
 * aligned; a segment whose four pointers are all 16-byte aligned moves 16 bytes per access.
 * Overlapping segments are the caller's error and are not checked.
 * WH_EINVAL: nseg outside 0 .. WH_ADAM_MAX_SEGS; h == NULL; for nseg > 0 segs == NULL; a segment with
 * count < 0 or, for count > 0, a NULL or misaligned pointer.  nseg = 0 and segments of count 0 are
 * WH_OK and touch nothing. */
typedef struct wh_adam_seg { float *p, *m, *v; const float* g; int64_t count; } wh_adam_seg;
typedef struct wh_adam_hyper {
  float beta1, omb1;      /* beta1, 1 - beta1 */
  float beta2, omb2;      /* beta2, 1 - beta2 */
  float eps;
  float step_size;        /* lr / (1 - beta1^t) */
  float sqrt_bc2;         /* sqrt(1 - beta2^t) */
} wh_adam_hyper;
#define WH_ADAM_MAX_SEGS 24
int wh_adam_step(int32_t nseg, const wh_adam_seg* segs, const wh_adam_hyper* h, void* stream);
/* wh_adam_step with the step count where the arithmetic runs.  One call advances `clock` and then
 * steps the tensors from clock->h, in stream order, with no host read: a one-lane launch ticks the
 * clock, the launch after it reads the table (no grid-wide barrier, no flag).  The tick, in double:
 *   t += 1 ;  beta1_t *= beta1 ;  beta2_t *= beta2
 *   h = {beta1, 1 - beta1, beta2, 1 - beta2, eps, lr / (1 - beta1_t), sqrt(1 - beta2_t)}
 * each value rounded to f32 once, no fused multiply-adds.  beta^t is a running product, not pow, so
 * that the engines agree bit for bit: IEEE double multiply, subtract, divide and sqrt are correctly
 * rounded on both.  Confirmed for gfx950 from the compiled tick (the divide and the square root are
 * the compiler's v_rcp_f64 / v_rsq_f64 Newton expansions with their v_div_scale / v_div_fmas /
 * v_div_fixup and exponent-scaling fix-ups, which round correctly; no v_fma on the products or the
 * subtractions) and by tests/test_gpu_sync_free.py, which holds the device's clock and tensors to the
 * host engine's bit for bit over 20 chained steps.  Against lr / (1 - beta1 ** t) and
 * sqrt(1 - beta2 ** t) computed with pow, h is equal at t = 1 and within one f32 ulp per field later
 * (the product differs from pow by about t * 2^-53 relative).  The element arithmetic is wh_adam_step's.
 * A fresh clock is {0, 1.0, 1.0, any h}.
 * WH_EINVAL: wh_adam_step's segment rules; clock == NULL or not 8-byte aligned.  nseg = 0 (and a call
 * whose segments are all empty) still ticks.  Both engines implement it. */
typedef struct wh_adam_clock {      /* device memory (host memory on the host engine), 8-byte aligned */
  int64_t t;                        /* steps taken; 0 to start */
  double beta1_t, beta2_t;          /* beta1^t, beta2^t as running products; 1.0 to start */
  wh_adam_hyper h;                  /* the table of step t, written by the tick */
} wh_adam_clock;
int wh_adam_step_clock(int32_t nseg, const wh_adam_seg* segs, wh_adam_clock* clock,
                       double lr, double beta1, double beta2, double eps, void* stream);

/* Library build identification (e.g. "warehouse_amd gfx950 <date>"). */
const char* wh_version(void);

/* Assert-mode builds (-DWH_CHECK) check SURVEY §5's invariants inside the kernels after every
 * state load, step and reset: exactly R open requests, live agents inside the grid, carried
 * targets on delivery cells, request bytes valid delivery indices, open mask == table, n <= slots.
 * out[4] = {violations, first failing env id, its failed-check bits, env-states checked}; clear
 * != 0 zeroes the counters.  Synchronises the current device.  WH_ENOTSUP in production builds. */
int wh_check_read(uint64_t* out, int32_t clear);

#ifdef __cplusplus
}
#endif
#endif /* WAREHOUSE_AMD_H */
