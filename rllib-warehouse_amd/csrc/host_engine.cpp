// host_engine.cpp -- the warehouse transition on host cores (g++), behind the same C ABI as the
// gfx950 library (include/warehouse_amd.h): libwarehouse_host.so.
//
// What it is for: BASELINE config 1 ("1 env ... via baseline/run.py on CPU, no GPU").  The drop-in
// `warehouse.Warehouse` runs on this engine when no HIP device is present, so baseline/run.py and
// scripts/train.py work unchanged on a GPU-less host.  It is product code written from the
// reference (warehouse/core.py:167-442, baseline/solvers.py:27-58) and the header's contracts
// (packed state layout, injected draws, the philox draw contract of the device kernels) -- not a
// translation of the test oracle, which it never calls.  Every pointer is host memory and `stream`
// is ignored.  Entry points the CPU has no use for (the policy network, the fragment operand, the
// two-stream sampler step wh_sampler_step_to, prepared launches, assert mode, the 16-lanes-per-env
// entries wh_*_wide) return WH_ENOTSUP;
// wh_sampler_step / wh_sampler_rollout run as policy + vector step per env.
//
// The state is the device's packed word planes (state[w * B + e]), so a state can move between the
// two engines with a plain copy, and the philox draws follow the device's stream layout word for
// word: a CPU rollout equals a GPU rollout bit for bit (tests/test_host_engine.py, tests/test_gpu_host_engine.py).
// Envs are independent; batches of many envs are split over host threads (OpenMP).
//
// Which calls are refused is not this engine's business: the config checks, the option rules and a
// step-family call reduced to one struct come from abi_args.h, which the gfx950 library uses too, so
// both refuse the same calls with the same codes (tests/test_abi_refusals.py).  What is written here
// is the transition, this engine's own limits (make_geo) and one per-env driver for the step family.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "abi_args.h"
#include "geometry.h"
#include "sac_formula.h"
#include "warehouse_amd.h"

namespace {

constexpr uint32_t IDLE = 0xFF00FF00u;   // target bytes of an agent word that carries nothing
constexpr int kMaxP = 64, kMaxA = 64;     // pickup / delivery points and agent slots per env (64-bit sets)
constexpr int kMaxD = 32;

enum Purpose : uint32_t { PUR_RESET = 1, PUR_REGEN = 2, PUR_POLICY = 3, PUR_RANDOM = 4 };

// ----------------------------------------------------------------------------- geometry
struct Geo : wh_abi::Shape {   // a valid config's sizes (abi_args.h) and this engine's tables
  int NV;
  int8_t cell[kMaxD][kMaxD];   // [x][y]: pickup index, -1 for other cells
  int px[kMaxP], py[kMaxP];    // pickup point cells (core.py:171-175)
  int dxc[kMaxP], dyc[kMaxP];  // delivery point cells (core.py:178-188)
  int vx[kMaxD * kMaxD], vy[kMaxD * kMaxD];   // spawn cells: interior, not a pickup, ascending (x, y)
};

// The tables of a valid config; what this engine cannot run (more points or agents than its 64-bit
// sets hold, racks that overlap) is WH_ENOTSUP.
int make_geo(const wh_abi::Shape& shape, Geo* g) {
  static_cast<wh_abi::Shape&>(*g) = shape;
  static_assert(kMaxD >= 32, "the ABI's largest area");
  if (g->P > kMaxP || g->DP > kMaxP || g->NA > kMaxA) return WH_ENOTSUP;
  if (wh_geo::racks_overlap(g->racks, g->NR)) return WH_ENOTSUP;
  memset(g->cell, -1, sizeof(g->cell));
  for (int j = 0; j < g->P; ++j) {
    const wh_geo::Cell c = wh_geo::pickup_cell(g->racks, g->NR, j);
    g->cell[c.x][c.y] = (int8_t)j;
    g->px[j] = c.x;
    g->py[j] = c.y;
  }
  for (int d = 0; d < g->DP; ++d) {
    const wh_geo::Cell c = wh_geo::delivery_cell(d, g->D);
    g->dxc[d] = c.x;
    g->dyc[d] = c.y;
  }
  g->NV = wh_geo::spawn_cells(g->racks, g->NR, g->D, [g, i = 0](int x, int y) mutable {
    g->vx[i] = x;
    g->vy[i++] = y;
  });
  return WH_OK;
}

int make_geo(const wh_config* c, Geo* g) {
  wh_abi::Shape shape;
  const int rc = wh_abi::check_config(c, &shape);
  return rc ? rc : make_geo(shape, g);
}

// ----------------------------------------------------------------------------- philox
// Philox4x32-10 (Salmon et al., SC'11); the device streams (include/warehouse_amd.h, RNG MODES):
// key (seed lo, seed hi), counter (global env id, episode, t, purpose << 24 | block).
struct U4 {
  uint32_t v[4];
};
U4 philox10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0;
    c1 = (uint32_t)p1;
    c2 = n2;
    c3 = (uint32_t)p0;
  }
  return U4{{c0, c1, c2, c3}};
}
inline uint32_t umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

struct Stream {   // words of one (env, episode, t, purpose) stream, one block cached
  uint32_t k0, k1, env, ep, t, purpose;
  int cur = -1;
  U4 blk{};
  uint32_t word(int j) {
    if ((j >> 2) != cur) {
      cur = j >> 2;
      blk = philox10(env, ep, t, (purpose << 24) | (uint32_t)cur, k0, k1);
    }
    return blk.v[j & 3];
  }
};

// ----------------------------------------------------------------------------- one env, unpacked
struct Env {
  uint32_t t, n, fresh, epi;
  int x[kMaxA], y[kMaxA], tg[kMaxA];   // position, delivery target index (-1: carries nothing)
  int pt[kMaxP];                        // request target of pickup point j (-1: none)
  uint32_t pe[kMaxP];                   // expiry byte of point j (the packed plane keeps it when closed)
};

void load(const Geo& g, const uint32_t* st, int64_t B, int64_t e, Env& s) {
  const uint32_t h = st[e];
  s.t = h & 0xFFFFu;
  s.n = std::min<uint32_t>((h >> 16) & 0xFFu, (uint32_t)g.NA);
  s.fresh = (h >> 24) & 1u;
  s.epi = st[B + e];
  for (int i = 0; i < g.NA; ++i) {
    const uint32_t w = st[(int64_t)(2 + i) * B + e];
    s.x[i] = (int)(w & 0xFFu);
    s.y[i] = (int)((w >> 16) & 0xFFu);
    const uint32_t dx = (w >> 8) & 0xFFu, dy = w >> 24;
    s.tg[i] = (dx == 0xFFu) ? -1 : wh_geo::delivery_index((int)dx, (int)dy, g.D);
  }
  const int PW = g.P / 4;
  for (int w = 0; w < PW; ++w) {
    const uint32_t tw = st[(int64_t)(2 + g.NA + w) * B + e], mw = st[(int64_t)(2 + g.NA + PW + w) * B + e];
    for (int b = 0; b < 4; ++b) {
      const uint32_t tb = (tw >> (8 * b)) & 0xFFu;
      s.pt[4 * w + b] = (tb == 0u || tb > (uint32_t)g.DP) ? -1 : (int)tb - 1;
      s.pe[4 * w + b] = (mw >> (8 * b)) & 0xFFu;
    }
  }
}

void store(const Geo& g, uint32_t* st, int64_t B, int64_t e, const Env& s) {
  st[e] = (s.t & 0xFFFFu) | (s.n << 16) | (s.fresh << 24);
  st[B + e] = s.epi;
  for (int i = 0; i < g.NA; ++i) {
    uint32_t w = IDLE;
    if ((uint32_t)i < s.n) {
      w = (uint32_t)s.x[i] | ((uint32_t)s.y[i] << 16);
      w |= s.tg[i] >= 0 ? ((uint32_t)g.dxc[s.tg[i]] << 8) | ((uint32_t)g.dyc[s.tg[i]] << 24) : IDLE;
    }
    st[(int64_t)(2 + i) * B + e] = w;
  }
  const int PW = g.P / 4;
  for (int w = 0; w < PW; ++w) {
    uint32_t tw = 0, mw = 0;
    for (int b = 0; b < 4; ++b) {
      const int j = 4 * w + b;
      tw |= (uint32_t)(s.pt[j] + 1) << (8 * b);
      mw |= (s.pe[j] & 0xFFu) << (8 * b);
    }
    st[(int64_t)(2 + g.NA + w) * B + e] = tw;
    st[(int64_t)(2 + g.NA + PW + w) * B + e] = mw;
  }
}

// ----------------------------------------------------------------------------- reset
// core.py:167-221; Train variants draw n first (variants.py:73-74).
void clear_requests(const Geo& g, Env& s) {
  for (int j = 0; j < g.P; ++j) {
    s.pt[j] = -1;
    s.pe[j] = 0;
  }
}

// Injected draws: accepted spawn cells, the R opened points and their targets in draw order.
void reset_injected(const Geo& g, Env& s, int64_t e, const wh_reset_draws& d) {
  const uint32_t n = d.n ? std::min<uint32_t>((uint32_t)d.n[e], (uint32_t)g.NA) : (uint32_t)g.NA;
  for (int i = 0; i < g.NA; ++i) {
    const bool live = (uint32_t)i < n;
    s.x[i] = live ? std::min<int>((int)(uint32_t)d.spawn[(e * g.NA + i) * 2], g.D - 1) : 0;
    s.y[i] = live ? std::min<int>((int)(uint32_t)d.spawn[(e * g.NA + i) * 2 + 1], g.D - 1) : 0;
    s.tg[i] = -1;
  }
  clear_requests(g, s);
  for (int j = 0; j < g.R; ++j) {
    const uint32_t sel = (uint32_t)d.pickups[e * g.R + j], tg = (uint32_t)d.targets[e * g.R + j];
    if (sel >= (uint32_t)g.P || tg >= (uint32_t)g.DP) continue;   // invalid injected draw: ignored
    s.pt[sel] = (int)tg;
    s.pe[sel] = (uint32_t)g.W & 0xFFu;   // opened at t = 0 with wait W
  }
  s.t = 0;
  s.n = n;
  s.fresh = 1;
  s.epi += 1;
}

// Philox draws, the device's word layout (RESET purpose, episode epi + 1, t = 0): word 0 the agent
// count (variable_n), words 1..NA the spawn cells (uniform over the NV spawn cells: the law of the
// reference's rejection loop, core.py:191-201), then per request j the pair (point, target): the
// points a uniform R-subset by Floyd's algorithm, the targets a uniform ordered R-tuple of distinct
// delivery points (core.py:213-221: choice(P, R) paired with choice(Dp, R)).
void reset_philox(const Geo& g, Env& s, uint32_t k0, uint32_t k1, uint32_t gid, bool variable_n) {
  const uint32_t ep = s.epi + 1u;
  Stream w{k0, k1, gid, ep, 0u, PUR_RESET};
  const int na = g.NA;
  const uint32_t n = variable_n ? 1u + umulhi(w.word(0), (uint32_t)na) : (uint32_t)na;
  for (int i = 0; i < na; ++i) {
    const uint32_t v = umulhi(w.word(1 + i), (uint32_t)g.NV);
    const bool live = (uint32_t)i < n;
    s.x[i] = live ? g.vx[v] : 0;
    s.y[i] = live ? g.vy[v] : 0;
    s.tg[i] = -1;
  }
  clear_requests(g, s);
  uint64_t taken = 0;
  uint32_t sel[kMaxP], rank[kMaxP];
  for (int j = 0; j < g.R; ++j) {
    const uint32_t m = (uint32_t)(g.P - g.R + j);
    const uint32_t r = umulhi(w.word(1 + na + 2 * j), m + 1u);
    sel[j] = (j > 0 && ((taken >> r) & 1ull)) ? m : r;
    taken |= 1ull << sel[j];
    rank[j] = umulhi(w.word(2 + na + 2 * j), (uint32_t)(g.DP - j));
  }
  // item j's target: the rank[j]-th delivery point not taken by items < j
  uint64_t used = 0;
  for (int j = 0; j < g.R; ++j) {
    uint32_t r = rank[j];
    int d = 0;
    for (;; ++d)
      if (!((used >> d) & 1ull) && r-- == 0) break;
    used |= 1ull << d;
    s.pt[sel[j]] = d;
    s.pe[sel[j]] = (uint32_t)g.W & 0xFFu;
  }
  s.t = 0;
  s.n = n;
  s.fresh = 1;
  s.epi = ep;
}

// ----------------------------------------------------------------------------- step
// core.py:267-368.  Entries: the action dict in iteration order (agent | (own action + 1) << 8; an
// entry without its own action takes actions[agent]; -1 = no entry), or every live agent in
// ascending order when `ord` is NULL.  Actions > 8 act as 4 (stay); the host binding wraps negative
// actions like Python's list indexing and rejects >= 9 before it gets here.
struct StepOut {
  float rew[kMaxA];
  bool done;
  int nin;
};

constexpr int PH_ALL = WH_PHASE_ALL, PH_PRE = WH_PHASE_PRE_REGEN, PH_REGEN = WH_PHASE_REGEN;

inline int move_dx(uint32_t a) { return (int)(a / 3u) - 1; }   // MOVES[a] = (a // 3 - 1, a % 3 - 1), core.py:38
inline int move_dy(uint32_t a) { return (int)(a % 3u) - 1; }

void move_phase(const Geo& g, Env& s, const int32_t* acts, const int32_t* ord, int ol) {
  bool occ[kMaxD][kMaxD] = {};   // rebuilt from the positions every step (core.py:275-276)
  for (uint32_t i = 0; i < s.n; ++i) occ[s.x[i]][s.y[i]] = true;
  // invalid moves (core.py:277, 293-297) as (from x, from y, to x, to y) bytes
  std::vector<uint32_t> invalid;
  auto key = [](int a, int b, int c, int d) { return (uint32_t)a | ((uint32_t)b << 8) | ((uint32_t)c << 16) | ((uint32_t)d << 24); };
  const int count = ord ? ol : (int)s.n;
  for (int k = 0; k < count; ++k) {
    int who;
    uint32_t a;
    if (ord) {
      const int32_t raw = ord[k];
      if (raw < 0) continue;
      who = raw & 0xFF;
      const uint32_t own = ((uint32_t)raw >> 8) & 0xFFu;
      if ((uint32_t)who >= s.n) continue;
      a = own ? own - 1u : (uint32_t)acts[who];
    } else {
      who = k;
      a = (uint32_t)acts[k];
    }
    if (a > 8u) a = 4u;
    const int px = s.x[who], py = s.y[who];
    int x = px + move_dx(a), y = py + move_dy(a);
    if (!(0 <= x && x < g.D)) x = px;   // core.py:284-287
    if (!(0 <= y && y < g.D)) y = py;
    if (occ[x][y] || std::find(invalid.begin(), invalid.end(), key(px, py, x, y)) != invalid.end()) continue;
    occ[px][py] = false;
    occ[x][y] = true;
    invalid.push_back(key(x, y, px, py));
    if (x != px && y != py) {
      invalid.push_back(key(x, py, px, y));
      invalid.push_back(key(px, y, x, py));
    }
    s.x[who] = x;
    s.y[who] = y;
  }
}

// the r-th (0-based) member of set m, ascending
int select_bit(uint64_t m, uint32_t r) {
  for (int j = 0; j < 64; ++j)
    if ((m >> j) & 1ull) {
      if (r == 0) return j;
      --r;
    }
  return -1;
}

void regenerate(const Geo& g, Env& s, const int32_t* regen, uint32_t k0, uint32_t k1, uint32_t gid) {
  uint64_t inactive = 0;
  int nin = 0;
  for (int j = 0; j < g.P; ++j)
    if (s.pt[j] < 0) {
      inactive |= 1ull << j;
      ++nin;
    }
  const int k = g.R - g.P + nin;   // core.py:339-341 (draws are consumed even when k = 0)
  const uint32_t exp = (s.t + (uint32_t)g.W) & 0xFFu;
  if (regen) {
    // injected: R positions into the ascending inactive list, then R targets (core.py:339-350)
    for (int j = 0; j < k && j < g.R; ++j) {
      const uint32_t rpos = (uint32_t)regen[j], tgi = (uint32_t)regen[g.R + j];
      if (rpos >= (uint32_t)nin || tgi >= (uint32_t)g.DP) continue;   // invalid draws are ignored
      const int sel = select_bit(inactive, rpos);
      s.pt[sel] = (int)tgi;
      s.pe[sel] = exp;
    }
    return;
  }
  // philox (REGEN purpose, words 2j / 2j + 1 = item j's point / target): an ordered k-subset of the
  // inactive points and k distinct targets, each uniform over what earlier items left
  Stream w{k0, k1, gid, s.epi, s.t, PUR_REGEN};
  uint64_t left = inactive, used = 0;
  for (int j = 0; j < k && j < g.R; ++j) {
    const int sel = select_bit(left, umulhi(w.word(2 * j), (uint32_t)(nin - j)));
    const int tgi = select_bit(~used & (g.DP >= 64 ? ~0ull : ((1ull << g.DP) - 1ull)), umulhi(w.word(2 * j + 1), (uint32_t)(g.DP - j)));
    left &= ~(1ull << sel);
    used |= 1ull << tgi;
    s.pt[sel] = tgi;
    s.pe[sel] = exp;
  }
}

StepOut step_env(const Geo& g, Env& s, const int32_t* acts, const int32_t* ord, int ol, const int32_t* regen,
                 uint32_t k0, uint32_t k1, uint32_t gid, int phase) {
  StepOut o{};
  for (int i = 0; i < g.NA; ++i) o.rew[i] = 0.0f;
  if (phase != PH_REGEN) {
    s.t = (s.t + 1u) & 0xFFFFu;                         // core.py:267
    move_phase(g, s, acts, ord, ol);                    // core.py:275-300
    for (int j = 0; j < g.P; ++j)                       // core.py:303-306: timers count to the expiry step
      if (s.pt[j] >= 0 && s.pe[j] == (s.t & 0xFFu)) s.pt[j] = -1;
    // pickups (core.py:309-335): every agent decides against the pre-pickup table, then the points
    // are cleared (two agents on one point both take its request)
    int taken[kMaxA];
    for (uint32_t i = 0; i < s.n; ++i) {
      const int c = g.cell[s.x[i]][s.y[i]];
      taken[i] = (c >= 0 && s.tg[i] < 0 && s.pt[c] >= 0) ? c : -1;
    }
    for (uint32_t i = 0; i < s.n; ++i)
      if (taken[i] >= 0) {
        s.tg[i] = s.pt[taken[i]];
        o.rew[i] = 1.0f;
      }
    for (uint32_t i = 0; i < s.n; ++i)
      if (taken[i] >= 0) s.pt[taken[i]] = -1;
    o.nin = 0;
    for (int j = 0; j < g.P; ++j) o.nin += s.pt[j] < 0;
  }
  if (phase != PH_PRE) regenerate(g, s, regen, k0, k1, gid);   // core.py:338-351
  if (phase != PH_REGEN) {
    for (uint32_t i = 0; i < s.n; ++i)                 // deliveries, core.py:354-368
      if (s.tg[i] >= 0 && s.x[i] == g.dxc[s.tg[i]] && s.y[i] == g.dyc[s.tg[i]]) {
        s.tg[i] = -1;
        o.rew[i] = 1.0f;   // (a pickup, interior, and a delivery, on the border, never share a step)
      }
    o.done = s.t >= (uint32_t)g.T;                     // core.py:438
    s.fresh = 0;
  }
  return o;
}

// ----------------------------------------------------------------------------- policy
// baseline/solvers.py:27-58 on the state: availability 0 (fresh reset, or carrying) -> the own
// delivery target (the null cell (D/2, D/2) after a reset, core.py:233-236), else the nearest open
// request (Manhattan, first minimum = lowest pickup index wins); step = clip(goal - pos, -1, 1).
// With probability p the action is uniform over the 9 moves (POLICY stream: word 2i the coin,
// 2i + 1 the move of agent i).  Random policy: RANDOM stream word i.
void policy_env(const Geo& g, const Env& s, int policy, float p, uint32_t k0, uint32_t k1, uint32_t gid,
                int32_t* out) {
  for (int i = 0; i < g.NA; ++i) out[i] = 4;
  if (policy == WH_POLICY_RANDOM) {
    Stream w{k0, k1, gid, s.epi, s.t, PUR_RANDOM};
    for (uint32_t i = 0; i < s.n; ++i) out[i] = (int32_t)umulhi(w.word((int)i), 9u);
    return;
  }
  const int nul = g.D / 2;
  Stream w{k0, k1, gid, s.epi, s.t, PUR_POLICY};
  for (uint32_t i = 0; i < s.n; ++i) {
    int gx = nul, gy = nul;
    if (!s.fresh) {
      if (s.tg[i] >= 0) {
        gx = g.dxc[s.tg[i]];
        gy = g.dyc[s.tg[i]];
      } else {
        int best = 1 << 30;
        for (int j = 0; j < g.P; ++j)
          if (s.pt[j] >= 0) {
            const int dist = std::abs(g.px[j] - s.x[i]) + std::abs(g.py[j] - s.y[i]);
            if (dist < best) {
              best = dist;
              gx = g.px[j];
              gy = g.py[j];
            }
          }
      }
    }
    const int sx = std::max(-1, std::min(1, gx - s.x[i])), sy = std::max(-1, std::min(1, gy - s.y[i]));
    out[i] = (sx + 1) * 3 + (sy + 1);
    if (p > 0.0f) {
      const float u = (float)(w.word(2 * (int)i) >> 8) * (1.0f / 16777216.0f);
      if (u < p) out[i] = (int32_t)umulhi(w.word(2 * (int)i + 1), 9u);
    }
  }
}

// ----------------------------------------------------------------------------- observation rows
// core.py:224-260 (fresh) / 371-432, in sorted gym-Dict key order: num_agents,
// other_availabilities, other_delivery_targets, other_positions, requests, self_availability,
// self_delivery_target, self_position.  other_delivery_targets drops row 1 for every agent after a
// step (core.py:428) and row i after a reset (core.py:256).  Rows of slots >= n are zero.
void observe_env(const Geo& g, const Env& s, float* rows) {
  const int R = g.R, L = g.L;
  const float nul = (float)(g.D / 2);
  float av[kMaxP], dt[kMaxP][2], ps[kMaxP][2], rq[kMaxP][4];
  for (int r = 0; r < R; ++r) {
    const bool live = (uint32_t)r < s.n;
    const bool carry = live && s.tg[r] >= 0;
    av[r] = (live && !s.fresh && !carry) ? 1.0f : 0.0f;
    dt[r][0] = (carry && !s.fresh) ? (float)g.dxc[s.tg[r]] : nul;
    dt[r][1] = (carry && !s.fresh) ? (float)g.dyc[s.tg[r]] : nul;
    ps[r][0] = live ? (float)s.x[r] : nul;
    ps[r][1] = live ? (float)s.y[r] : nul;
  }
  int q = 0;
  for (int j = 0; j < g.P && q < R; ++j)
    if (s.pt[j] >= 0) {
      rq[q][0] = (float)g.px[j];
      rq[q][1] = (float)g.py[j];
      rq[q][2] = (float)g.dxc[s.pt[j]];
      rq[q][3] = (float)g.dyc[s.pt[j]];
      ++q;
    }
  for (; q < R; ++q) rq[q][0] = rq[q][1] = rq[q][2] = rq[q][3] = 0.0f;
  for (int i = 0; i < g.NA; ++i) {
    float* o = rows + (int64_t)i * L;
    if ((uint32_t)i >= s.n) {
      memset(o, 0, sizeof(float) * L);
      continue;
    }
    int f = 0;
    o[f++] = (float)s.n;
    for (int r = 0; r < R; ++r)
      if (r != i) o[f++] = av[r];
    const int drop = s.fresh ? i : 1;
    for (int r = 0; r < R; ++r)
      if (r != drop) {
        o[f++] = dt[r][0];
        o[f++] = dt[r][1];
      }
    for (int r = 0; r < R; ++r)
      if (r != i) {
        o[f++] = ps[r][0];
        o[f++] = ps[r][1];
      }
    for (int r = 0; r < R; ++r)
      for (int c = 0; c < 4; ++c) o[f++] = rq[r][c];
    o[f++] = av[i];
    o[f++] = dt[i][0];
    o[f++] = dt[i][1];
    o[f++] = ps[i][0];
    o[f++] = ps[i][1];
  }
}

// ----------------------------------------------------------------------------- episode metrics
void fold_episode(const wh_episode_stats* st, uint32_t n, uint32_t ret) {
  if (!st) return;
#pragma omp critical(wh_host_stats)
  {
    if (st->return_sum) st->return_sum[n] += ret;
    if (st->episodes) st->episodes[n] += 1;
    if (st->return_min) st->return_min[n] = std::min(st->return_min[n], ret);
    if (st->return_max) st->return_max[n] = std::max(st->return_max[n], ret);
  }
}

// ----------------------------------------------------------------------------- the step family
// One env of a checked step-family call (abi_args.h): c.steps times [policy ->] step -> rewards /
// dones -> episode-return fold -> auto-reset on an unmasked env, then its rows.  wh_step (phases,
// injected regeneration draws), wh_rollout (a policy, K steps, returns), wh_vector_step (a mask,
// rows) and wh_sampler_step (a policy, rows) are this with the options each one sets.  With a ring
// (wh_replay_record) every step is recorded: the env's record and actions before the step, its
// record, rewards and done flag after it and before the reset.
void drive_env(const Geo& g, const wh_abi::StepCall& c, int64_t e) {
  const int64_t B = c.B;
  const uint32_t k0 = wh_abi::lo32(c.seed), k1 = wh_abi::hi32(c.seed), gid = (uint32_t)(c.env_offset + e);
  Env s;
  load(g, c.state, B, e, s);
  if (!c.mask || c.mask[e]) {
    const bool st = c.stats && c.stats->episode_return;
    uint32_t epr = st ? c.stats->episode_return[e] : 0u;
    float ret = 0.0f;
    int32_t acts[kMaxA];
    for (int k = 0; k < c.steps; ++k) {
      const int32_t* a = c.actions ? c.actions + e * g.NA : nullptr;
      if (c.policy != wh_abi::POLICY_EXTERNAL) {
        policy_env(g, s, c.policy, c.p, k0, k1, gid, acts);
        a = acts;
      }
      // the ring entry of this step, and its side-0 record ((slot * 2 + side) * B + e)
      const int64_t ent = c.ring ? ((c.slot + k) % c.ring->capacity) * B + e : 0;
      uint32_t* rec = c.ring ? c.ring->states + (2 * ent - e) * g.words : nullptr;
      if (c.ring) {
        // side 0: the words just loaded (step 0), else the state the previous step (and reset) left
        if (k == 0)
          for (int w = 0; w < g.words; ++w) rec[w] = c.state[(int64_t)w * B + e];
        else
          store(g, rec, 1, 0, s);   // (a record is a one-env word-plane state)
        for (int i = 0; i < g.NA; ++i) {
          const uint32_t act = (uint32_t)a[i];
          c.ring->actions[ent * g.NA + i] = (uint8_t)(act > 8u ? 4u : act);
        }
      }
      const StepOut o = step_env(g, s, a, c.order ? c.order + e * c.ol : nullptr, c.ol,
                                 c.regen ? c.regen + e * 2 * g.R : nullptr, k0, k1, gid, c.phase);
      const int64_t row = (int64_t)k * B + e;
      float r = 0.0f;
      for (int i = 0; i < g.NA; ++i) r += o.rew[i];
      if (c.ring) {   // side 1: the stepped state, before any reset
        store(g, rec + B * g.words, 1, 0, s);
        for (int i = 0; i < g.NA; ++i) c.ring->rewards[ent * g.NA + i] = o.rew[i];
        c.ring->dones[ent] = o.done ? 1 : 0;
      }
      if (c.phase != WH_PHASE_REGEN) {
        if (c.rewards)
          for (int i = 0; i < g.NA; ++i) c.rewards[row * g.NA + i] = o.rew[i];
        if (c.dones) c.dones[row] = o.done ? 1 : 0;
      }
      if (c.phase == WH_PHASE_PRE_REGEN && c.n_inactive) c.n_inactive[e] = o.nin;
      ret += r;
      if (st) {
        epr += (uint32_t)r;
        if (o.done) {
          fold_episode(c.stats, s.n, epr);
          epr = 0;
        }
      }
      if (o.done && c.autoreset) reset_philox(g, s, k0, k1, gid, c.variable_n != 0);
    }
    if (c.returns) c.returns[e] += ret;
    if (st) c.stats->episode_return[e] = epr;
    store(g, c.state, B, e, s);
  }
  if (c.obs) observe_env(g, s, c.obs + e * g.NA * g.L);
}

// every env of the call, over host threads from `par_min` envs on
void run_envs(const Geo& g, const wh_abi::StepCall& c, int64_t par_min) {
#pragma omp parallel for schedule(static) if (c.B >= par_min)
  for (int64_t e = 0; e < c.B; ++e) drive_env(g, c, e);
}

int run_call(int rc, const wh_abi::StepCall& c, int64_t par_min = 1024) {
  Geo g;
  if (rc || (rc = make_geo(c.g, &g))) return rc;
  run_envs(g, c, par_min);
  return WH_OK;
}

}  // namespace

// =============================================================================== C ABI
extern "C" {

int wh_query(const wh_config* cfg, wh_layout* out) {
  Geo g;
  const int rc = make_geo(cfg, &g);
  if (rc) return rc;
  if (out) {
    out->words_per_env = g.words;
    out->num_pickups = g.P;
    out->num_deliveries = g.DP;
    out->obs_len = g.L;
    out->kernel_agents = g.NA;
  }
  return WH_OK;
}

int wh_pack(const wh_config* cfg, int64_t B, const int32_t* pos, const int32_t* agent_target,
            const int32_t* pickup_target, const int32_t* pickup_timer, const int32_t* t, const int32_t* n,
            const uint8_t* fresh, const uint32_t* episode, uint32_t* state, void* stream) {
  (void)stream;
  Geo g;
  int rc = wh_abi::pack_call(&g, cfg, B, state, pos, agent_target, pickup_target, pickup_timer, t, n, fresh, episode);
  if (rc || (rc = make_geo(wh_abi::Shape(g), &g)) || B == 0) return rc;
  for (int64_t e = 0; e < B; ++e) {   // out-of-range canonical values are clamped (as wh_pack on the device)
    Env s{};
    s.t = (uint32_t)t[e] & 0xFFFFu;
    s.n = (uint32_t)std::min(std::max(n[e], 0), g.NA);
    s.fresh = fresh[e] ? 1u : 0u;
    s.epi = episode[e];
    for (int i = 0; i < g.NA; ++i) {
      s.x[i] = std::min(std::max(pos[(e * g.NA + i) * 2], 0), g.D - 1);
      s.y[i] = std::min(std::max(pos[(e * g.NA + i) * 2 + 1], 0), g.D - 1);
      const int32_t tg = agent_target[e * g.NA + i];
      s.tg[i] = (tg >= 0 && tg < g.DP) ? tg : -1;
    }
    for (int j = 0; j < g.P; ++j) {
      const int32_t tg = pickup_target[e * g.P + j];
      s.pt[j] = (tg >= 0 && tg < g.DP) ? tg : -1;
      s.pe[j] = s.pt[j] >= 0 ? ((uint32_t)t[e] + (uint32_t)pickup_timer[e * g.P + j]) & 0xFFu : 0u;
    }
    store(g, state, B, e, s);
  }
  return WH_OK;
}

int wh_unpack(const wh_config* cfg, int64_t B, const uint32_t* state, int32_t* pos, int32_t* agent_target,
              int32_t* pickup_target, int32_t* pickup_timer, int32_t* t, int32_t* n, uint8_t* fresh,
              uint32_t* episode, void* stream) {
  (void)stream;
  Geo g;
  int rc = wh_abi::pack_call(&g, cfg, B, state, pos, agent_target, pickup_target, pickup_timer, t, n, fresh, episode);
  if (rc || (rc = make_geo(wh_abi::Shape(g), &g)) || B == 0) return rc;
  for (int64_t e = 0; e < B; ++e) {
    Env s;
    load(g, state, B, e, s);
    t[e] = (int32_t)s.t;
    n[e] = (int32_t)((state[e] >> 16) & 0xFFu);
    fresh[e] = (uint8_t)s.fresh;
    episode[e] = s.epi;
    for (int i = 0; i < g.NA; ++i) {
      const bool live = (uint32_t)i < s.n;
      pos[(e * g.NA + i) * 2] = live ? s.x[i] : 0;
      pos[(e * g.NA + i) * 2 + 1] = live ? s.y[i] : 0;
      agent_target[e * g.NA + i] = live ? s.tg[i] : -1;
    }
    for (int j = 0; j < g.P; ++j) {
      pickup_target[e * g.P + j] = s.pt[j];
      pickup_timer[e * g.P + j] = s.pt[j] >= 0 ? (int32_t)((s.pe[j] - s.t) & 0xFFu) : -1;   // steps left
    }
  }
  return WH_OK;
}

int wh_reset(const wh_config* cfg, int64_t B, uint32_t* state, const uint8_t* mask, const wh_reset_draws* draws,
             int32_t variable_n, uint64_t seed, int64_t env_offset, void* stream) {
  (void)stream;
  Geo g;
  int rc = wh_abi::reset_call(&g, cfg, B, state, draws);
  if (rc || (rc = make_geo(wh_abi::Shape(g), &g)) || B == 0) return rc;
#pragma omp parallel for schedule(static) if (B >= 1024)
  for (int64_t e = 0; e < B; ++e) {
    if (mask && !mask[e]) continue;
    Env s;
    load(g, state, B, e, s);
    if (draws)
      reset_injected(g, s, e, *draws);
    else
      reset_philox(g, s, wh_abi::lo32(seed), wh_abi::hi32(seed), (uint32_t)(env_offset + e), variable_n != 0);
    store(g, state, B, e, s);
  }
  return WH_OK;
}

int wh_step(const wh_config* cfg, int64_t B, uint32_t* state, const int32_t* actions, const int32_t* order,
            int32_t order_len, float* rewards, uint8_t* dones, const int32_t* regen, int32_t* n_inactive,
            int32_t phase, uint64_t seed, int64_t env_offset, void*) {
  wh_abi::StepCall c;
  return run_call(wh_abi::step_call(&c, cfg, B, state, actions, order, order_len, rewards, dones, regen, n_inactive,
                                    phase, seed, env_offset, 1), c);
}

int wh_observe(const wh_config* cfg, int64_t B, const uint32_t* state, float* obs, void*) {
  Geo g;
  int rc = wh_abi::observe_call(&g, cfg, B, state, obs, nullptr);
  if (rc || (rc = make_geo(wh_abi::Shape(g), &g)) || B == 0) return rc;
#pragma omp parallel for schedule(static) if (B >= 1024)
  for (int64_t e = 0; e < B; ++e) {
    Env s;
    load(g, state, B, e, s);
    observe_env(g, s, obs + e * g.NA * g.L);
  }
  return WH_OK;
}

int wh_policy(const wh_config* cfg, int64_t B, const uint32_t* state, int32_t policy, float p, int32_t* actions,
              uint64_t seed, int64_t env_offset, void*) {
  wh_abi::StepCall c;
  Geo g;
  int rc = wh_abi::policy_call(&c, cfg, B, state, policy, p, actions, seed, env_offset);
  if (rc || (rc = make_geo(c.g, &g))) return rc;
#pragma omp parallel for schedule(static) if (B >= 1024)
  for (int64_t e = 0; e < B; ++e) {
    Env s;
    load(g, state, B, e, s);
    policy_env(g, s, policy, p, wh_abi::lo32(seed), wh_abi::hi32(seed), (uint32_t)(env_offset + e), actions + e * g.NA);
  }
  return WH_OK;
}

int wh_rollout(const wh_config* cfg, int64_t B, uint32_t* state, int32_t steps, int32_t policy, float p,
               float* rewards, uint8_t* dones, float* returns, const wh_episode_stats* stats, int32_t autoreset,
               int32_t variable_n, uint64_t seed, int64_t env_offset, void*) {
  wh_abi::StepCall c;
  return run_call(wh_abi::rollout_call(&c, cfg, B, state, steps, policy, p, rewards, dones, returns, stats, autoreset,
                                       variable_n, seed, env_offset, 1), c, 256);
}

int wh_vector_step(const wh_config* cfg, int64_t B, uint32_t* state, const int32_t* actions, const int32_t* order,
                   int32_t order_len, const uint8_t* mask, float* rewards, uint8_t* dones, float* obs,
                   const wh_episode_stats* stats, int32_t autoreset, int32_t variable_n, uint64_t seed,
                   int64_t env_offset, void*) {
  wh_abi::StepCall c;
  return run_call(wh_abi::vector_step_call(&c, cfg, B, state, actions, order, order_len, mask, rewards, dones, obs,
                                           nullptr, false, stats, autoreset, variable_n, seed, env_offset, 1), c);
}

// policy + vector step per env (every env stepped, auto-reset)
int wh_sampler_step(const wh_config* cfg, int64_t B, uint32_t* state, int32_t policy, float p, float* rewards,
                    uint8_t* dones, float* obs, const wh_episode_stats* stats, int32_t variable_n, uint64_t seed,
                    int64_t env_offset, void*) {
  wh_abi::StepCall c;
  return run_call(wh_abi::sampler_step_call(&c, cfg, B, state, nullptr, false, policy, p, rewards, dones, obs, stats,
                                            variable_n, seed, env_offset), c);
}

// `steps` sampler steps over the whole batch, the rows of every step kept
int wh_sampler_rollout(const wh_config* cfg, int64_t B, uint32_t* state, int32_t steps, int32_t policy, float p,
                       float* rewards, uint8_t* dones, float* obs, const wh_episode_stats* stats, int32_t variable_n,
                       uint64_t seed, int64_t env_offset, void*) {
  wh_abi::StepCall c;
  Geo g;
  int rc = wh_abi::sampler_rollout_call(&c, cfg, B, state, steps, policy, p, rewards, dones, obs, stats, variable_n,
                                        seed, env_offset);
  if (rc || (rc = make_geo(c.g, &g))) return rc;
  c.steps = 1;
  for (int32_t k = 0; k < steps; ++k) {
    run_envs(g, c, 1024);
    if (c.rewards) c.rewards += B * g.NA;
    if (c.dones) c.dones += B;
    if (c.obs) c.obs += B * g.NA * g.L;
  }
  return WH_OK;
}

// ---- replay ring (include/warehouse_amd.h, REPLAY RING): the device's layout, index draw and
// invalid-index rule; the rows come from observe_env
int wh_replay_put(const wh_config* cfg, int64_t B, const wh_replay_ring* ring, int64_t slot, int32_t stage,
                  const uint32_t* state, const int32_t* actions, const float* rewards, const uint8_t* dones, void*) {
  Geo g;
  int rc = wh_abi::replay_put_call(&g, cfg, B, ring, slot, stage, state, actions, rewards, dones);
  if (rc || (rc = make_geo(wh_abi::Shape(g), &g))) return rc;
  if (B == 0) return WH_OK;
  const int words = g.words, na = g.NA;
  uint32_t* rec = ring->states + (2 * slot + stage) * B * words;
#pragma omp parallel for schedule(static) if (B >= 1024)
  for (int64_t e = 0; e < B; ++e) {
    for (int w = 0; w < words; ++w) rec[e * words + w] = state[(int64_t)w * B + e];
    if (stage == 0) {
      for (int i = 0; i < na; ++i) {
        const uint32_t a = (uint32_t)actions[e * na + i];
        ring->actions[(slot * B + e) * na + i] = (uint8_t)(a > 8u ? 4u : a);
      }
    } else {
      for (int i = 0; i < na; ++i) ring->rewards[(slot * B + e) * na + i] = rewards[e * na + i];
      ring->dones[slot * B + e] = dones[e];
    }
  }
  return WH_OK;
}

// `steps` recorded steps per env (drive_env with a ring), then the rows of the final state
int wh_replay_record(const wh_config* cfg, int64_t B, uint32_t* state, const wh_replay_ring* ring, int64_t slot,
                     int32_t steps, int32_t policy, float p, const int32_t* actions, float* rewards, uint8_t* dones,
                     float* obs, void* xfrag, const wh_episode_stats* stats, int32_t variable_n, uint64_t seed,
                     int64_t env_offset, void*) {
  wh_abi::StepCall c;
  Geo g;
  int rc = wh_abi::replay_record_call(&c, cfg, B, state, ring, slot, steps, policy, p, actions, rewards, dones, obs,
                                      xfrag, stats, variable_n, seed, env_offset);
  if (rc || (rc = make_geo(c.g, &g))) return rc;
  if (xfrag) return WH_ENOTSUP;   // the fragment operand is a device format
  if (B == 0 || steps == 0) return WH_OK;
  run_envs(g, c, 1024);
  return WH_OK;
}

int wh_replay_gather(const wh_config* cfg, int64_t B, const wh_replay_ring* ring, int64_t filled, int64_t M,
                     const int64_t* idx, uint64_t seed, uint64_t draw, const wh_replay_batch* b, void*) {
  Geo g;
  int rc = wh_abi::replay_gather_call(&g, cfg, B, ring, filled, M, b);
  if (rc || (rc = make_geo(wh_abi::Shape(g), &g))) return rc;
  if (wh_abi::batch_has_frags(b)) return WH_ENOTSUP;   // the fragment operand is a device format
  if (B == 0 || M == 0) return WH_OK;
  const int words = g.words, na = g.NA;
  const int64_t row = (int64_t)na * g.L;
  const uint32_t k0 = wh_abi::lo32(seed), k1 = wh_abi::hi32(seed);
#pragma omp parallel for schedule(static) if (M >= 1024)
  for (int64_t m = 0; m < M; ++m) {
    int64_t ix;
    if (idx) {
      ix = idx[m];
      if (ix < 0 || ix >= filled * B) ix = -1;
    } else {
      const U4 r = philox10((uint32_t)m, (uint32_t)(draw & 0xFFFFFFFFu), (uint32_t)(draw >> 32), 6u << 24, k0, k1);
      ix = (int64_t)(((uint64_t)r.v[0] * (uint64_t)filled) >> 32) * B + (int64_t)(((uint64_t)r.v[1] * (uint64_t)B) >> 32);
    }
    const int64_t slot = ix < 0 ? 0 : ix / B;
    uint32_t side_n = 0;
    for (int side = 0; side < 2; ++side) {
      float* rows = side ? b->next_obs : b->obs;
      uint32_t* planes = side ? b->next_state : b->state;
      // an invalid index reads nothing: an all-zero record (n = 0, zero rows)
      std::vector<uint32_t> rec((size_t)words, 0u);
      if (ix >= 0) memcpy(rec.data(), ring->states + (ix + (slot + side) * B) * words, sizeof(uint32_t) * words);
      if (planes)
        for (int w = 0; w < words; ++w) planes[(int64_t)w * M + m] = rec[w];
      if (rows || side == 0) {
        Env s;
        load(g, rec.data(), 1, 0, s);   // (a record is a one-env word-plane state)
        if (side == 0) side_n = s.n;
        if (rows) observe_env(g, s, rows + m * row);
      }
    }
    for (int i = 0; i < na; ++i) {
      if (b->actions) b->actions[m * na + i] = ix < 0 ? 0 : (int32_t)ring->actions[ix * na + i];
      if (b->rewards) b->rewards[m * na + i] = ix < 0 ? 0.0f : ring->rewards[ix * na + i];
    }
    if (b->dones) b->dones[m] = ix < 0 ? 0 : ring->dones[ix];
    if (b->n) b->n[m] = ix < 0 ? -1 : (int32_t)side_n;
    if (b->idx_out) b->idx_out[m] = ix < 0 ? 0 : ix;
  }
  return WH_OK;
}

// ---- replay priorities (include/warehouse_amd.h, REPLAY PRIORITIES): the device's layout and
// rules in plain serial loops -- integer sums, so the tree is the device's bit for bit
static void prio_add(const wh_replay_prio* t, const wh_abi::PrioShape& s, int64_t leaf, uint64_t delta) {
  for (int k = 1; k <= s.levels; ++k) t->node[s.off[k] + (leaf >> (4 * k))] += delta;   // (wrapping: a signed delta)
}

int wh_replay_prio_query(int64_t count, int64_t* leaf_words, int64_t* node_words, int32_t* levels) {
  return wh_abi::prio_query(count, leaf_words, node_words, levels);
}

int wh_replay_prio_fill(const wh_replay_prio* tree, int64_t first, int64_t n, int32_t mode, uint32_t q, void*) {
  wh_abi::PrioShape s;
  const int rc = wh_abi::prio_fill_call(&s, tree, first, n, mode, q);
  if (rc || n == 0) return rc;
  if (mode) q = *tree->max_q;
  for (int64_t i = first; i < first + n; ++i) {
    const uint64_t delta = (uint64_t)q - (uint64_t)tree->leaf[i];
    tree->leaf[i] = q;
    if (delta) prio_add(tree, s, i, delta);
  }
  return WH_OK;
}

int wh_replay_prio_update(const wh_replay_prio* tree, int64_t M, const int64_t* idx, const float* p, void*) {
  wh_abi::PrioShape s;
  const int rc = wh_abi::prio_update_call(&s, tree, M, idx, p);
  if (rc || M == 0) return rc;
  // clear every touched leaf, then raise it to the largest q given for it
  for (int64_t m = 0; m < M; ++m) {
    const int64_t i = idx[m];
    if (i < 0 || i >= tree->count || !tree->leaf[i]) continue;
    prio_add(tree, s, i, 0ull - (uint64_t)tree->leaf[i]);
    tree->leaf[i] = 0;
  }
  uint32_t qmax = *tree->max_q;
  for (int64_t m = 0; m < M; ++m) {
    const int64_t i = idx[m];
    if (i < 0 || i >= tree->count) continue;
    const uint32_t q = wh_abi::prio_quantise(p[m]);
    qmax = std::max(qmax, q);
    if (q <= tree->leaf[i]) continue;
    prio_add(tree, s, i, (uint64_t)(q - tree->leaf[i]));
    tree->leaf[i] = q;
  }
  *tree->max_q = qmax;
  return WH_OK;
}

int wh_replay_prio_sample(const wh_replay_prio* tree, int64_t M, const uint64_t* u, uint64_t seed, uint64_t draw,
                          int64_t* idx_out, uint32_t* q_out, uint64_t* total_out, void*) {
  wh_abi::PrioShape s;
  const int rc = wh_abi::prio_sample_call(&s, tree, M, idx_out);
  if (rc || M == 0) return rc;
  const uint32_t k0 = wh_abi::lo32(seed), k1 = wh_abi::hi32(seed);
  const uint64_t total = tree->node[s.off[s.levels]];
  if (total_out) *total_out = total;
  for (int64_t m = 0; m < M; ++m) {
    uint64_t r;
    if (u) {
      r = u[m];
    } else {
      const U4 w = philox10((uint32_t)m, (uint32_t)(draw & 0xFFFFFFFFu), (uint32_t)(draw >> 32), 7u << 24, k0, k1);
      r = (uint64_t)w.v[0] << 32 | w.v[1];
    }
    uint64_t mass = (uint64_t)(((unsigned __int128)r * total) >> 64);
    int64_t pos = 0;
    uint32_t q = 0;
    for (int k = s.levels - 1; k >= 0; --k) {
      // the first child whose inclusive prefix exceeds the mass (none: the last, as the device does)
      uint64_t ex = 0;
      int j = 0;
      for (;; ++j) {
        const uint64_t v = k ? tree->node[s.off[k] + pos * 16 + j] : (uint64_t)tree->leaf[pos * 16 + j];
        q = (uint32_t)v;
        if (ex + v > mass || j == 15) break;
        ex += v;
      }
      mass -= ex;
      pos = std::min(pos * 16 + j, s.n[k] - 1);
    }
    idx_out[m] = total ? pos : -1;
    if (q_out) q_out[m] = total ? q : 0u;
  }
  return WH_OK;
}

// ---- SAC TD targets (include/warehouse_amd.h, SAC TD TARGETS): sac_formula.h's arithmetic, the
// device's operation order, in a plain loop over the rows
int wh_sac_td(int64_t M, int32_t NA, const wh_sac_td_args* a, void*) {
  const int rc = wh_abi::sac_td_call(M, NA, a);
  if (rc || M == 0) return rc;
  const bool twin = a->q2 != nullptr;
  for (int64_t m = 0; m < M; ++m) {
    const int nn = wh_sac::live_rows(a->n, m, NA);
    const bool masked = a->mask_dones != 0 && a->dones[m] != 0;
    float sum = 0.0f;
    for (int i = 0; i < NA; ++i) {
      const int64_t row = m * NA + i, e = row * wh_sac::OUT;
      float y = 0.0f, tdr = 0.0f;
      if (i < nn) {
        const float v = wh_sac::soft_value(a->pi_next + e, a->q1t_next + e, a->q2t_next ? a->q2t_next + e : nullptr, a->alpha);
        y = wh_sac::target(a->rewards[row], a->discount, masked, v);
        if (a->q1) {
          const int act = wh_sac::taken_action(a->actions[row]);
          tdr = wh_sac::td_row(a->q1[e + act], twin ? a->q2[e + act] : 0.0f, twin, y);
        }
      }
      if (a->y) a->y[row] = y;
      if (a->td_rows) a->td_rows[row] = tdr;
      sum += tdr;
    }
    if (a->td) a->td[m] = wh_sac::td_mean(sum, nn);
  }
  return WH_OK;
}

// alpha = expf(log_alpha[0]), as wh_sac_loss below forms it; the rest is wh_sac_td
int wh_sac_td_la(int64_t M, int32_t NA, const wh_sac_td_args* a, const float* log_alpha, void* stream) {
  const int rc = wh_abi::sac_td_la_call(M, NA, a, log_alpha);
  if (rc || M == 0) return rc;
  wh_sac_td_args b = *a;
  b.alpha = expf(log_alpha[0]);
  return wh_sac_td(M, NA, &b, stream);
}

// ---- SAC losses (include/warehouse_amd.h, SAC LOSSES): sac_formula.h's row arithmetic, the sums in
// ascending row order; `work` is checked like the device's and not used
int wh_sac_loss_query(int64_t M, int32_t NA, int64_t* work_bytes) { return wh_abi::sac_loss_query_call(M, NA, work_bytes); }

int wh_sac_loss(int64_t M, int32_t NA, const wh_sac_loss_args* a, void*) {
  const int rc = wh_abi::sac_loss_call(M, NA, a);
  if (rc || M == 0) return rc;
  const bool twin = a->q2 != nullptr;
  const float alpha = expf(a->log_alpha[0]);
  float sums[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int64_t m = 0; m < M; ++m) {
    const int nn = wh_sac::live_rows(a->n, m, NA);
    const float w = a->weights ? a->weights[m] : 1.0f;
    for (int i = 0; i < NA; ++i) {
      const int64_t row = m * NA + i, e = row * wh_sac::OUT;
      float dpi[wh_sac::OUT] = {};
      float d1 = 0.0f, d2 = 0.0f;
      int act = -1;
      if (i < nn) {
        act = wh_sac::taken_action(a->actions[row]);
        const wh_sac::LossRow r = wh_sac::loss_row(a->pi + e, a->q1 + e, twin ? a->q2 + e : nullptr, twin, a->y[row], act,
                                                   w, alpha, a->target_entropy, a->scale, dpi);
        d1 = wh_sac::loss_dq(a->scale, w, r.e1);
        d2 = twin ? wh_sac::loss_dq(a->scale, w, r.e2) : 0.0f;
        sums[0] += r.c1;
        sums[1] += r.c2;
        sums[2] += r.f;
        sums[3] += r.t;
        sums[4] += 1.0f;
      }
      for (int o = 0; o < wh_sac::OUT; ++o) {
        if (a->dpi) a->dpi[e + o] = dpi[o];
        if (a->dq1) a->dq1[e + o] = o == act ? d1 : 0.0f;
        if (a->dq2) a->dq2[e + o] = o == act ? d2 : 0.0f;
      }
    }
  }
  wh_sac::loss_stats(sums, a->scale, a->log_alpha[0], a->stats);
  return WH_OK;
}

// ---- Adam (include/warehouse_amd.h, ADAM): sac_formula.h's element, segment after segment
int wh_adam_step(int32_t nseg, const wh_adam_seg* segs, const wh_adam_hyper* h, void*) {
  const int rc = wh_abi::adam_call(nseg, segs, h);
  if (rc) return rc;
  for (int32_t s = 0; s < nseg; ++s) {
    const wh_adam_seg& g = segs[s];
    for (int64_t e = 0; e < g.count; ++e) wh_sac::adam_element(*h, g.g[e], g.p[e], g.m[e], g.v[e]);
  }
  return WH_OK;
}

// the tick (sac_formula.h's adam_tick, the device's), then the step from the table it wrote
int wh_adam_step_clock(int32_t nseg, const wh_adam_seg* segs, wh_adam_clock* clock, double lr, double beta1,
                       double beta2, double eps, void* stream) {
  const int rc = wh_abi::adam_clock_call(nseg, segs, clock);
  if (rc) return rc;
  wh_sac::adam_tick(*clock, lr, beta1, beta2, eps);
  return wh_adam_step(nseg, segs, &clock->h, stream);
}

// ---- what the CPU has no use for: the policy network and its fragment operand (device formats),
// the two-stream sampler step, prepared launches, assert-mode counters, and the 16-lanes-per-env
// form (csrc/step_wide.h: the host engine has no lanes)
int wh_observe_x(const wh_config*, int64_t, const uint32_t*, float*, void*, void*) { return WH_ENOTSUP; }
int wh_vector_step_x(const wh_config*, int64_t, uint32_t*, const int32_t*, const int32_t*, int32_t, const uint8_t*,
                     float*, uint8_t*, void*, const wh_episode_stats*, int32_t, int32_t, uint64_t, int64_t, void*) { return WH_ENOTSUP; }
int wh_sampler_step_to(const wh_config*, int64_t, const uint32_t*, uint32_t*, int32_t, float, float*, uint8_t*,
                       const wh_episode_stats*, int32_t, uint64_t, int64_t, void*) { return WH_ENOTSUP; }
int wh_rollout_prepare(const wh_config*, int64_t, uint32_t*, int32_t, int32_t, float, float*, uint8_t*, float*,
                       const wh_episode_stats*, int32_t, int32_t, uint64_t, int64_t, void*, wh_launch** out) {
  if (out) *out = nullptr;
  return WH_ENOTSUP;
}
int wh_launch_run(const wh_launch*) { return WH_EINVAL; }   // (no handle is ever live here)
int wh_launch_run_timed(const wh_launch*, void*, void*) { return WH_EINVAL; }
int wh_launch_free(wh_launch* launch) { return launch ? WH_EINVAL : WH_OK; }
int wh_mlp_query(const wh_mlp_desc*, int64_t*) { return WH_ENOTSUP; }
int wh_mlp_pack(const wh_mlp_desc*, const float*, const float*, const float*, const float*, const float*,
                const float*, void*) { return WH_ENOTSUP; }
int wh_mlp_pack_device(const wh_mlp_desc*, const float*, const float*, const float*, const float*, const float*,
                       const float*, void*, void*) { return WH_ENOTSUP; }
int wh_mlp_forward(const wh_mlp_desc*, const void*, int64_t, const float*, float*, int32_t*, int32_t, uint64_t,
                   uint32_t, void*) { return WH_ENOTSUP; }
int wh_mlp_forward_x(const wh_mlp_desc*, const void*, int64_t, const void*, float*, int32_t*, int32_t, uint64_t,
                     uint32_t, void*) { return WH_ENOTSUP; }
int wh_mlp_forward_multi(const wh_mlp_desc*, int32_t, const wh_mlp_job*, void*) { return WH_ENOTSUP; }
int wh_mlp_train_query(const wh_mlp_desc*, int64_t, int64_t*) { return WH_ENOTSUP; }
int wh_mlp_train_forward(const wh_mlp_desc*, const wh_mlp_weights*, int64_t, const float*, float*, float*, float*,
                         void*) { return WH_ENOTSUP; }
int wh_mlp_backward(const wh_mlp_desc*, const wh_mlp_weights*, int64_t, const float*, const float*, const float*,
                    const float*, const wh_mlp_grads*, void*, void*) { return WH_ENOTSUP; }
int wh_mlp_train_forward_multi(const wh_mlp_desc*, int32_t, const wh_mlp_train_job*, int64_t, void*) { return WH_ENOTSUP; }
int wh_mlp_backward_multi(const wh_mlp_desc*, int32_t, const wh_mlp_train_job*, int64_t, void*) { return WH_ENOTSUP; }
int wh_check_read(uint64_t*, int32_t) { return WH_ENOTSUP; }
int wh_step_wide(const wh_config*, int64_t, uint32_t*, const int32_t*, float*, uint8_t*, const int32_t*, int32_t*,
                 uint64_t, int64_t, int32_t, void*) { return WH_ENOTSUP; }
int wh_rollout_wide(const wh_config*, int64_t, uint32_t*, int32_t, int32_t, float, float*, uint8_t*, float*,
                    const wh_episode_stats*, int32_t, int32_t, uint64_t, int64_t, int32_t, void*) { return WH_ENOTSUP; }
int wh_vector_step_wide(const wh_config*, int64_t, uint32_t*, const int32_t*, const uint8_t*, float*, uint8_t*, float*,
                        const wh_episode_stats*, int32_t, int32_t, uint64_t, int64_t, int32_t, void*) { return WH_ENOTSUP; }

}  // extern "C"
