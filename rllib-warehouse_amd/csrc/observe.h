// observe.h -- the observation rows (device code; included by warehouse_amd.hip after step_env.h,
// whose obs_src it builds its gather tables from): ObsSrc, the row and fragment writers
// (stream_rows, stream_frags), the image build from the packed state, k_observe.
//
// Observation rows (core.py:371-432, reset rows core.py:224-260), HBM-write bound.
// Each env's values live in a small byte image whose layout is one row's value pool:
//   [0] n, [1..R] availability, R x (x,y) delivery targets, R x (x,y) positions,
//   R x (px,py,dx,dy) requests (active slots, ascending pickup index).
// Output float k of an env (k = i*L + f for agent row i, feature f) is img[src[fresh][k]] when
// i < n, else 0.  src is a compile-time byte table per (R, NAM): every row's "other agents"
// gather (skip row i; other_delivery_targets skips row 1 unless the episode is fresh, core.py:428
// vs :256) is folded into it, so the write loop is branch-free.  A workgroup images 16 envs with
// 16 lanes per env, then writes the group's contiguous [16 env x na x L] float region as float4s.
// Small workgroups keep many groups in flight per CU, so one group's image build overlaps the
// others' streaming stores.

template <int R, int NAM>
struct ObsSrc {
  static constexpr int L = 9 * R + 1, W = (NAM * L + 3) / 4;
  uint32_t w[2][W];
};
template <int R, int NAM, int A0 = 1, int G0 = 1 + R, int P0 = 1 + 3 * R, int Q0 = 1 + 5 * R>
constexpr ObsSrc<R, NAM> make_obs_src() {
  ObsSrc<R, NAM> t{};
  constexpr int L = 9 * R + 1;
  for (int fr = 0; fr < 2; ++fr)
    for (int k = 0; k < NAM * L; ++k)
      t.w[fr][k >> 2] |= obs_src<R, A0, G0, P0, Q0>(k / L, k % L, fr != 0) << (8 * (k & 3));
  return t;
}
template <int R, int NAM>
__constant__ ObsSrc<R, NAM> kObsSrc = make_obs_src<R, NAM>();

// The rows [nenv x na x L] f32 of a group's envs from their LDS byte images, float4 q per lane of
// NT lanes (per env: qe float4s, lim = live floats | fresh << 31, gather bytes from src0 / src1 by
// freshness).  Every LDS read is unconditional -- a dead value reads a byte of the image (or past the
// LDS object, which returns 0 without a fault) and is selected away: the conditional form compiled
// to a branch and an lgkmcnt(0) round trip per float, four serial LDS latencies per store.  Both
// gather words are read beside lim, so a float4 takes two LDS round trips, and RU float4s per lane
// are in flight together.
#ifndef WH_ROWS_RU
#define WH_ROWS_RU 2
#endif
template <int NT, int IMG, bool NTS, int RU = WH_ROWS_RU>
__device__ __forceinline__ void stream_rows(const uint32_t* lims, const uint32_t* src0, const uint32_t* src1,
                                            const uint8_t* img, f32x4* __restrict__ out4, uint32_t nenv,
                                            uint32_t qe, int tid, uint32_t q0 = 0, uint32_t q1 = ~0u) {
  const uint32_t magic = 0xFFFFFFFFu / qe + 1u;   // q / qe == umulhi(q, magic) while q * qe < 2^32
  const uint32_t total = nenv * qe < q1 ? nenv * qe : q1;   // float4s [q0, total) of the group
  for (uint32_t q = q0 + tid; q < total; q += RU * NT) {
    f32x4 v[RU];
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const uint32_t qu = q + (uint32_t)u * NT < total ? q + (uint32_t)u * NT : q;
      const uint32_t el4 = __umulhi(qu, magic);
      const uint32_t k4 = qu - el4 * qe;
      const uint32_t lim = lims[el4];
      const uint32_t s0 = src0[k4], s1 = src1[k4];
      const uint32_t sw = (int32_t)lim < 0 ? s1 : s0;
      const int lv = (int)(lim & 0x7FFFFFFFu) - 4 * (int)k4;   // > j  <=>  value j is live
      const uint8_t* im = img + el4 * IMG;
      const uint32_t b0 = im[sw & 0xFFu], b1 = im[(sw >> 8) & 0xFFu], b2 = im[(sw >> 16) & 0xFFu],
                     b3 = im[sw >> 24];
      v[u].x = lv > 0 ? (float)b0 : 0.0f;
      v[u].y = lv > 1 ? (float)b1 : 0.0f;
      v[u].z = lv > 2 ? (float)b2 : 0.0f;
      v[u].w = lv > 3 ? (float)b3 : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const uint32_t qu = q + (uint32_t)u * NT;
      if (u == 0 || qu < total) {
        if constexpr (NTS) __builtin_nontemporal_store(v[u], &out4[qu]);
        else out4[qu] = v[u];
      }
    }
  }
}

// The same rows as the policy network's layer-0 B operand (wh_observe_x's layout, below) for the
// group's envs [e0, e0 + nenv), from the images: NT lanes, 16 bytes of whole 32-row tiles each
// (the group's rows nenv * na are whole tiles except in a tail group).  src0 / src1: the gather
// tables (fresh / not fresh: lim's top bit), img: IMG bytes per env.
template <int NT, int L, int IMG>
__device__ __forceinline__ void stream_frags(const uint32_t* lims, const uint32_t* src0, const uint32_t* src1,
                                             const uint8_t* img, uint4* __restrict__ xfrag, int64_t e0,
                                             uint32_t nenv, int na, int tid) {
  constexpr int KQ = (L + 2 + 15) / 16;
  const uint32_t rows = nenv * (uint32_t)na, tiles = (rows + 31u) / 32u;   // (a tail group: fewer)
  // row / na == umulhi(row, magic) while row * na < 2^32, for na >= 2; for na == 1 the constant
  // 2^32 wraps to 0, so that case takes the row itself (every env but the first of a
  // group read env 0's image)
  const bool one = na == 1;
  const uint32_t magic = one ? 0u : 0xFFFFFFFFu / (uint32_t)na + 1u;
  uint4* out = xfrag + ((e0 * na) / 32) * (int64_t)(KQ * 64);
  for (uint32_t c = tid; c < tiles * KQ * 64; c += NT) {
    const uint32_t lane = c & 63u, tq = c >> 6, q = tq % KQ, t = tq / KQ;
    const uint32_t row = t * 32u + (lane & 31u);   // counted from the group's first env
    const uint32_t el1 = one ? row : __umulhi(row, magic), i = row - el1 * (uint32_t)na;
    const bool rl = row < rows;
    const uint32_t lim = lims[rl ? el1 : 0];
    const bool live_row = rl && i < ((lim & 0x7FFFFFFFu) / L);
    const uint8_t* sb = reinterpret_cast<const uint8_t*>((int32_t)lim < 0 ? src1 : src0);
    const uint8_t* im = img + (rl ? el1 : 0) * IMG;
    // unconditional gathers (see stream_rows): the index of a padding feature (k >= L) reads a
    // gather byte past the row, or past the table, and is selected away
    const uint32_t k0 = 16u * q + 8u * (lane >> 5);
    uint32_t gb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) gb[j] = sb[i * L + k0 + j];
    uint32_t w[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      uint32_t hv[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const uint32_t k = k0 + 2u * jj + u;
        const float x = (float)im[gb[2 * jj + u]];
        const float v = k < (uint32_t)L ? (live_row ? x : 0.0f) : (k < (uint32_t)L + 2u ? 1.0f : 0.0f);
        hv[u] = __float_as_uint(v) >> 16;   // byte values and 1.0: exact in bf16
      }
      w[jj] = hv[0] | (hv[1] << 16);
    }
    typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
    const u32x4v v = {w[0], w[1], w[2], w[3]};
    *reinterpret_cast<u32x4v*>(&out[c]) = v;   // plain: the policy network reads it next (see rows_nt)
  }
}

template <class C, int OBS_EB>
struct ObsLds {
  static constexpr int IMG = (C::L + 3) & ~3;
  static constexpr int SRCW = ObsSrc<C::R, C::NAM>::W;
  uint8_t img[OBS_EB][IMG];
  uint32_t lim[OBS_EB];          // n * L (floats of live rows) | fresh << 31
  uint32_t ptw[OBS_EB][C::PW];   // pickup target words (nonzero byte = active slot)
  uint32_t src[2][SRCW];
  uint32_t rp[C::P];             // pickup cell, x | y << 16
  uint32_t dst[C::DP];           // delivery cell, x << 8 | y << 24 | 0x00FF00FF
};

// The image build, shared by k_observe and k_replay_gather (replay.h).  It is written against a WORD
// SOURCE: a callable w -> word w of this lane's env.  k_observe reads the live state's word planes
// (PlaneWords: state[w * B + e]); the replay gather reads a record it has staged in LDS.  The build is
// split where k_observe's barriers fall: issue the tables and the env's words (every global load
// before its first use), commit the tables and write the agent rows and the pickup words, then (after
// a barrier) the popcount-ranked requests.
struct PlaneWords {
  const uint32_t* st;
  int64_t B, e;
  __device__ __forceinline__ uint32_t operator()(int w) const { return st[w * B + e]; }
};

template <class C>
struct ObsTabRegs {   // the per-workgroup tables in flight: gather table, pickup cells, delivery cells
  static constexpr int SRCW = ObsSrc<C::R, C::NAM>::W;
  static constexpr int NSRC = (2 * SRCW + BT - 1) / BT, NRP = (C::P + BT - 1) / BT, NDP = (C::DP + BT - 1) / BT;
  uint32_t sv[NSRC], rv[NRP], dv[NDP];
};
template <class C>
__device__ __forceinline__ void obs_tables_issue(ObsTabRegs<C>& t, const uint32_t* tables, int tid) {
  using T = ObsTabRegs<C>;
  const uint32_t* srcg = &kObsSrc<C::R, C::NAM>.w[0][0];
#pragma unroll
  for (int i = 0; i < T::NSRC; ++i) t.sv[i] = tid + i * BT < 2 * T::SRCW ? srcg[tid + i * BT] : 0u;
#pragma unroll
  for (int i = 0; i < T::NRP; ++i) t.rv[i] = tid + i * BT < C::P ? tables[C::T.rp / 4 + 2 * (tid + i * BT)] : 0u;
#pragma unroll
  for (int i = 0; i < T::NDP; ++i) t.dv[i] = tid + i * BT < C::DP ? tables[C::T.dst / 4 + tid + i * BT] : 0u;
}
template <class C, int OBS_EB>
__device__ __forceinline__ void obs_tables_commit(ObsLds<C, OBS_EB>& O, const ObsTabRegs<C>& t, int tid) {
  using T = ObsTabRegs<C>;
#pragma unroll
  for (int i = 0; i < T::NSRC; ++i)
    if (tid + i * BT < 2 * T::SRCW) (&O.src[0][0])[tid + i * BT] = t.sv[i];
#pragma unroll
  for (int i = 0; i < T::NRP; ++i)
    if (tid + i * BT < C::P) O.rp[tid + i * BT] = t.rv[i];
#pragma unroll
  for (int i = 0; i < T::NDP; ++i)
    if (tid + i * BT < C::DP) O.dst[tid + i * BT] = t.dv[i];
}

template <class C, int OBS_EB>
struct ObsEnvWords {   // this lane's share of its env's words: OBS_PARTS lanes per env
  static constexpr int OBS_PARTS = BT / OBS_EB;
  static constexpr int NAR = (C::R + OBS_PARTS - 1) / OBS_PARTS, NPW = (C::PW + OBS_PARTS - 1) / OBS_PARTS;
  uint32_t av[NAR], pv[NPW], hdr;
};
// An agent row past n is loaded and replaced by IDLE in the image (rows r < na exist in the state).
template <class C, int OBS_EB, class WORDS>
__device__ __forceinline__ void obs_words_issue(ObsEnvWords<C, OBS_EB>& r, const WORDS& word, int part, int na) {
  using E = ObsEnvWords<C, OBS_EB>;
  r.hdr = word(0);
#pragma unroll
  for (int i = 0; i < E::NAR; ++i) {
    const int a = part + i * E::OBS_PARTS;
    r.av[i] = (a < C::R && a < na) ? word(2 + a) : IDLE;
  }
#pragma unroll
  for (int i = 0; i < E::NPW; ++i) {
    const int w = part + i * E::OBS_PARTS;
    r.pv[i] = w < C::PW ? word(2 + na + w) : 0u;
  }
}
// agent rows, n, lim and the pickup words of env slot `el` (a barrier follows)
template <class C, int OBS_EB>
__device__ __forceinline__ void obs_image_agents(ObsLds<C, OBS_EB>& O, const ObsEnvWords<C, OBS_EB>& r, int el,
                                                 int part, int na) {
  using E = ObsEnvWords<C, OBS_EB>;
  constexpr int R = C::R, D = C::D, L = C::L;
  constexpr int A0 = 1, G0 = 1 + R, P0 = 1 + 3 * R;
  const uint8_t nul = (uint8_t)(D / 2);
  uint32_t n = (r.hdr >> 16) & 0xFFu;
  n = n < (uint32_t)na ? n : (uint32_t)na;
  const bool fresh = (r.hdr >> 24) & 1u;
  uint8_t* im = O.img[el];
  if (part == 0) {
    im[0] = (uint8_t)n;
    O.lim[el] = n * L | (fresh ? 0x80000000u : 0u);
  }
#pragma unroll
  for (int i = 0; i < E::NAR; ++i) {                       // agent rows
    const int ar = part + i * E::OBS_PARTS;
    if (ar < R) {
      const bool live = ar < (int)n;
      const uint32_t a = live ? r.av[i] : IDLE;
      const bool carry = (a & 0xFF00u) != 0xFF00u;
      im[A0 + ar] = (uint8_t)((live && !fresh && !carry) ? 1 : 0);
      const bool show = live && !fresh && carry;
      im[G0 + 2 * ar] = show ? (uint8_t)((a >> 8) & 0xFFu) : nul;
      im[G0 + 2 * ar + 1] = show ? (uint8_t)(a >> 24) : nul;
      im[P0 + 2 * ar] = live ? (uint8_t)(a & 0xFFu) : nul;
      im[P0 + 2 * ar + 1] = live ? (uint8_t)((a >> 16) & 0xFFu) : nul;
    }
  }
#pragma unroll
  for (int i = 0; i < E::NPW; ++i) {
    const int w = part + i * E::OBS_PARTS;
    if (w < C::PW) O.ptw[el][w] = r.pv[i];
  }
}
// requests of env slot `el`: ascending pickup index, ranked by the popcount of the words before
template <class C, int OBS_EB>
__device__ __forceinline__ void obs_image_requests(ObsLds<C, OBS_EB>& O, int el, int part) {
  constexpr int R = C::R, Q0 = 1 + 5 * R, OBS_PARTS = BT / OBS_EB;
  uint8_t* im = O.img[el];
  for (int w = part; w < C::PW; w += OBS_PARTS) {
    uint32_t r = 0;
    for (int v = 0; v < w; ++v) r += __popc(nz_hi(O.ptw[el][v]));
    const uint32_t pt = O.ptw[el][w];
    for (int b = 0; b < 4; ++b) {
      const uint32_t tg = (pt >> (8 * b)) & 0xFFu;
      if (tg && r < (uint32_t)R) {
        const uint32_t pxy = O.rp[4 * w + b];
        const uint32_t dxy = O.dst[(tg - 1u) % C::DP];   // x << 8 | y << 24 (| 0x00FF00FF)
        im[Q0 + 4 * r] = (uint8_t)(pxy & 0xFFu);
        im[Q0 + 4 * r + 1] = (uint8_t)(pxy >> 16);
        im[Q0 + 4 * r + 2] = (uint8_t)(dxy >> 8);
        im[Q0 + 4 * r + 3] = (uint8_t)(dxy >> 24);
        ++r;
      }
    }
    if (w == C::PW - 1)      // fewer than R active slots never occurs after reset/step; keep rows defined
      for (; r < (uint32_t)R; ++r)
        im[Q0 + 4 * r] = im[Q0 + 4 * r + 1] = im[Q0 + 4 * r + 2] = im[Q0 + 4 * r + 3] = 0;
  }
}
// the rows of a group whose env rows are not whole float4s (or not 16-byte aligned): one float per lane
template <class C, int OBS_EB>
__device__ __forceinline__ void stream_rows_scalar(const ObsLds<C, OBS_EB>& O, float* out, uint32_t nenv,
                                                   uint32_t per_env, int tid) {
  const uint32_t total = nenv * per_env;
  const uint32_t magic = 0xFFFFFFFFu / per_env + 1u;
  for (uint32_t o = tid; o < total; o += BT) {
    const uint32_t el1 = __umulhi(o, magic);
    const uint32_t k = o - el1 * per_env;
    const uint32_t lim = O.lim[el1];
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(O.src[lim >> 31]);
    out[o] = k < (lim & 0x7FFFFFFFu) ? (float)O.img[el1][sb[k]] : 0.0f;
  }
}

// xfrag (optional): the same rows as the policy network's layer-0 B operand (policy_mlp.hip),
// bf16, in MFMA fragment order: 16-byte chunk ((tile * KQ + q) * 64 + lane) of agent-row tile
// `tile` (32 rows) holds features 16q + 8h + j (j < 8) of row tile*32 + (lane & 31), h = lane >> 5;
// features L, L+1 are 1.0 (the MLP's bias columns), the rest of the padding 0.  One coalesced
// 16-byte load per k-step for the MLP instead of scattered f32 rows (and half the bytes).
// CHUNK > 0 (f32 rows as whole float4s only): workgroup c writes the CHUNK float4s [c * CHUNK,
// (c + 1) * CHUNK) of the flat rows instead of its own envs' rows, imaging the (at most OBS_EB) envs
// they belong to -- smaller regions per workgroup, which the write path takes faster (constant
// stores: 16 KB per workgroup 100 us against 37 KB 113 us for Large-16's 608 MB,
// profiles/r06_obs_write_probe_chunks.txt).
template <class C, int OBS_EB, int CHUNK = 0>
__global__ __launch_bounds__(BT) void k_observe(const uint32_t* __restrict__ state, int64_t B, int na,
                                                const uint32_t* __restrict__ tables,
                                                float* __restrict__ obs, int quads,
                                                uint4* __restrict__ xfrag) {
  __shared__ ObsLds<C, OBS_EB> O;
  constexpr int OBS_PARTS = BT / OBS_EB;
  constexpr int L = C::L;
  const int tid = threadIdx.x;
  int64_t e0;
  uint32_t nenv, qlo = 0, qhi = ~0u;
  if constexpr (CHUNK > 0) {
    const int64_t qe = (int64_t)na * L / 4;
    const int64_t qa = (int64_t)blockIdx.x * CHUNK, qb = min(qa + CHUNK, B * qe);
    e0 = qa / qe;
    nenv = (uint32_t)((qb - 1) / qe - e0 + 1);   // <= OBS_EB (observe_impl: CHUNK <= (OBS_EB - 1) * qe + 1)
    qlo = (uint32_t)(qa - e0 * qe);
    qhi = (uint32_t)(qb - e0 * qe);
  } else {
    e0 = (int64_t)blockIdx.x * OBS_EB;
    nenv = (uint32_t)((B - e0) < OBS_EB ? (B - e0) : OBS_EB);
  }
  const int el = tid / OBS_PARTS, part = tid % OBS_PARTS;
  const bool mine = (uint32_t)el < nenv;
  const int64_t e = e0 + el;
  // Every global load of the prologue is issued before its first use: as strided loops, each
  // iteration compiled to a load -> vmcnt(0) -> LDS write round trip, and the agent rows waited on
  // the header (their guard was r < n) -- about eight serial memory latencies per workgroup for
  // Large-16 (five for its 4.6 KB gather table alone), now one.
  ObsTabRegs<C> tr;
  ObsEnvWords<C, OBS_EB> ew;
  ew.hdr = 0;
  obs_tables_issue<C>(tr, tables, tid);
  if (mine) obs_words_issue<C, OBS_EB>(ew, PlaneWords{state, B, e}, part, na);
  obs_tables_commit<C, OBS_EB>(O, tr, tid);
  if (mine) obs_image_agents<C, OBS_EB>(O, ew, el, part, na);
  __syncthreads();
  if (mine) obs_image_requests<C, OBS_EB>(O, el, part);
  __syncthreads();
  const uint32_t per_env = (uint32_t)na * L;
  if (xfrag)   // the group's rows are whole 32-row tiles (OBS_EB * na % 32 == 0, checked on the host)
    stream_frags<BT, L, ObsLds<C, OBS_EB>::IMG>(O.lim, O.src[0], O.src[1], &O.img[0][0], xfrag, e0, nenv, na, tid);
  if (!obs) return;
  float* out = obs + e0 * per_env;
  if (quads) {
    // per_env % 4 == 0 and obs 16-byte aligned (checked on the host)
    // (the chunk form: all of a lane's float4s in flight together)
    constexpr int RU = CHUNK > 0 ? (CHUNK / BT < 1 ? 1 : (CHUNK / BT > 4 ? 4 : CHUNK / BT)) : WH_ROWS_RU;
    stream_rows<BT, ObsLds<C, OBS_EB>::IMG, rows_nt<C>(), RU>(O.lim, O.src[0], O.src[1], &O.img[0][0],
                                                              reinterpret_cast<f32x4*>(out), nenv, per_env >> 2, tid,
                                                              qlo, qhi);
  } else {
    stream_rows_scalar<C, OBS_EB>(O, out, nenv, per_env, tid);
  }
}
