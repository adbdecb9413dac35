// replay.h -- the replay ring's two kernels (include/warehouse_amd.h, REPLAY RING).  Included by
// warehouse_amd.hip inside its namespace, after k_observe: the gather reuses k_observe's image build
// (obs_tables_*, obs_words_issue, obs_image_*) and its row writers (stream_rows, stream_frags).
//
// A ring stores a transition as two packed states, env-major: record ((slot * 2 + side) * B + e) is
// the `words` consecutive words of env e.  A sampled transition then reads one contiguous 56 / 112 /
// 200 byte record per side; the live state's word-plane-major layout would cost `words` scattered
// 4-byte reads per side, at sector granularity about as many bytes as the rows the gather writes.
// The transpose is paid once, at record time (k_replay_put), where both sides are coalesced.

// j / d for small d through a multiply: magic = 2^32 / d rounded up, exact while j * d < 2^32; the
// constant wraps to 0 for d == 1, which takes j itself (stream_frags' na == 1 case)
struct SmallDiv {
  uint32_t d, magic;
  __device__ __forceinline__ explicit SmallDiv(uint32_t d_) : d(d_), magic(d_ == 1u ? 0u : 0xFFFFFFFFu / d_ + 1u) {}
  __device__ __forceinline__ uint32_t operator()(uint32_t j) const { return d == 1u ? j : __umulhi(j, magic); }
};

// ----------------------------------------------------------------------------- put
struct PutParams {
  const uint32_t* state;   // live [words, B]
  uint32_t* rec;           // records of (slot, side): [B, words]
  int64_t B;
  int words, na;
  const int32_t* actions;  // stage 0: [B, NA] -> r_actions (u8), else null
  uint8_t* r_actions;
  const float* rewards;    // stage 1: [B, NA] -> r_rewards, [B] -> r_dones, else null
  float* r_rewards;
  const uint8_t* dones;
  uint8_t* r_dones;
};

// One workgroup transposes BT envs through LDS: lane = env reads every word plane (coalesced, all
// loads issued before the first LDS write), then the group's records -- contiguous in the ring --
// are written as consecutive words.  The LDS row is padded to an odd word count, so the plane-side
// writes (lane stride = one row) spread over every bank instead of landing in gcd(row, banks) of them.
template <class C>
__global__ __launch_bounds__(BT) void k_replay_put(PutParams a) {
  constexpr int WMAX = 2 + C::NAM + 2 * C::PW, STRIDE = WMAX | 1;
  __shared__ uint32_t tile[BT * STRIDE];
  const int tid = threadIdx.x;
  const int64_t e0 = (int64_t)blockIdx.x * BT;
  const uint32_t nenv = (uint32_t)((a.B - e0) < BT ? (a.B - e0) : BT);
  const bool mine = (uint32_t)tid < nenv;
  uint32_t v[WMAX];
#pragma unroll
  for (int w = 0; w < WMAX; ++w) v[w] = (mine && w < a.words) ? a.state[w * a.B + e0 + tid] : 0u;
#pragma unroll
  for (int w = 0; w < WMAX; ++w)
    if (w < a.words) tile[tid * STRIDE + w] = v[w];
  __syncthreads();
  const uint32_t total = nenv * (uint32_t)a.words;
  const SmallDiv by_words((uint32_t)a.words);
  uint32_t* out = a.rec + e0 * a.words;
  for (uint32_t j = tid; j < total; j += BT) {
    const uint32_t el = by_words(j), w = j - el * (uint32_t)a.words;
    out[j] = tile[el * STRIDE + w];
  }
  const uint32_t per = nenv * (uint32_t)a.na;
  const int64_t r0 = e0 * a.na;
  if (a.actions)
    for (uint32_t j = tid; j < per; j += BT) {
      const uint32_t act = (uint32_t)a.actions[r0 + j];
      a.r_actions[r0 + j] = (uint8_t)(act > 8u ? 4u : act);   // (what the step does with such a value)
    }
  if (a.rewards)
    for (uint32_t j = tid; j < per; j += BT) a.r_rewards[r0 + j] = a.rewards[r0 + j];
  if (a.dones && mine) a.r_dones[e0 + tid] = a.dones[e0 + tid];
}

// ----------------------------------------------------------------------------- gather
struct GatherParams {
  const uint32_t* states;   // the ring
  const uint8_t* r_actions;
  const float* r_rewards;
  const uint8_t* r_dones;
  int64_t B, filled, M;
  const int64_t* idx;       // [M] or null (philox, purpose 6)
  uint32_t k0, k1, d0, d1;  // seed and draw, low / high words
  int na, words, quads;
  unsigned groups;          // workgroups per side: ceil(M / EB)
  const uint32_t* tables;
  float* obs[2];            // [side]
  uint4* xfrag[2];
  uint32_t* state[2];
  int32_t* actions;
  float* rewards;
  uint8_t* dones;
  int32_t* n;
  int64_t* idx_out;
};

constexpr uint32_t PUR_REPLAY = 6;

template <class C, int EB>
struct ReplayLds {
  static constexpr int WMAX = 2 + C::NAM + 2 * C::PW;
  ObsLds<C, EB> O;
  int64_t rec[EB];          // record of this side: (slot * 2 + side) * B + env, -1 = invalid index
  int64_t ix[EB];           // the index itself, slot * B + env, -1 = invalid
  uint32_t words[EB][WMAX];
};

struct RecWords {   // the word source of the image build: a record staged in LDS
  const uint32_t* rec;
  __device__ __forceinline__ uint32_t operator()(int w) const { return rec[w]; }
};

// Workgroup (side, group) images samples [group * EB, +EB) of one side as k_observe images EB envs,
// and streams their rows through the same writers: side 0 to obs / xfrag, side 1 to next_obs /
// next_xfrag.  Order of the prologue: resolve the group's indices (explicit or philox) -> issue every
// record word, small-output and table load -> stage the records in LDS -> image.  An invalid index
// takes the same path with a predicated load: its record is all zero words, whose image is n = 0,
// lim = 0, hence zero rows; nothing branches around the imaging.
template <class C, int EB>
__global__ __launch_bounds__(BT) void k_replay_gather(GatherParams a) {
  __shared__ ReplayLds<C, EB> S;
  ObsLds<C, EB>& O = S.O;
  constexpr int PARTS = BT / EB, L = C::L, WMAX = ReplayLds<C, EB>::WMAX;
  constexpr int NREC = (EB * WMAX + BT - 1) / BT, NACT = (EB * C::NAM + BT - 1) / BT;
  const int tid = threadIdx.x;
  const unsigned side = blockIdx.x >= a.groups ? 1u : 0u, grp = blockIdx.x - side * a.groups;
  const int64_t e0 = (int64_t)grp * EB;
  const uint32_t nenv = (uint32_t)((a.M - e0) < EB ? (a.M - e0) : EB);
  const uint32_t na = (uint32_t)a.na, wpe = (uint32_t)a.words;

  ObsTabRegs<C> tr;
  obs_tables_issue<C>(tr, a.tables, tid);
  if (tid < EB) {
    int64_t ix = -1, slot = 0;
    if ((uint32_t)tid < nenv) {
      const int64_t m = e0 + tid;
      if (a.idx) {
        ix = a.idx[m];
        if (ix < 0 || ix >= a.filled * a.B) ix = -1;
        slot = ix < 0 ? 0 : ix / a.B;
      } else {
        const uint4 r = philox10(make_uint4((uint32_t)m, a.d0, a.d1, PUR_REPLAY << 24), a.k0, a.k1);
        slot = (int64_t)(((uint64_t)r.x * (uint64_t)a.filled) >> 32);
        ix = slot * a.B + (int64_t)(((uint64_t)r.y * (uint64_t)a.B) >> 32);
      }
      if (side == 0 && a.idx_out) a.idx_out[m] = ix < 0 ? 0 : ix;
    }
    S.ix[tid] = ix;
    S.rec[tid] = ix < 0 ? -1 : ix + (slot + (int64_t)side) * a.B;
  }
  __syncthreads();

  // every load of the group, before the first use
  const uint32_t total = nenv * wpe, rows = nenv * na;
  const SmallDiv by_words(wpe), by_na(na);
  uint32_t rv[NREC];
#pragma unroll
  for (int i = 0; i < NREC; ++i) {
    const uint32_t j = tid + i * BT, el = by_words(j), w = j - el * wpe;
    const int64_t rb = j < total ? S.rec[el] : -1;
    rv[i] = rb >= 0 ? a.states[rb * wpe + w] : 0u;
  }
  uint32_t act[NACT], dn = 0;
  float rw[NACT];
  if (side == 0) {
#pragma unroll
    for (int i = 0; i < NACT; ++i) {
      const uint32_t j = tid + i * BT, el = by_na(j), ag = j - el * na;
      const int64_t ix = j < rows ? S.ix[el] : -1;
      act[i] = (ix >= 0 && a.actions) ? a.r_actions[ix * na + ag] : 0u;
      rw[i] = (ix >= 0 && a.rewards) ? a.r_rewards[ix * na + ag] : 0.0f;
    }
    const int64_t ix = (uint32_t)tid < nenv ? S.ix[tid] : -1;
    dn = (ix >= 0 && a.dones) ? a.r_dones[ix] : 0u;
  }
#pragma unroll
  for (int i = 0; i < NREC; ++i) {
    const uint32_t j = tid + i * BT, el = by_words(j), w = j - el * wpe;
    if (j < total) S.words[el][w] = rv[i];
  }
  obs_tables_commit<C, EB>(O, tr, tid);
  if (side == 0) {
#pragma unroll
    for (int i = 0; i < NACT; ++i) {
      const uint32_t j = tid + i * BT;
      if (j < rows) {
        if (a.actions) a.actions[e0 * na + j] = (int32_t)act[i];
        if (a.rewards) a.rewards[e0 * na + j] = rw[i];
      }
    }
    if (a.dones && (uint32_t)tid < nenv) a.dones[e0 + tid] = (uint8_t)dn;
  }
  __syncthreads();

  const int el = tid / PARTS, part = tid % PARTS;
  const bool mine = (uint32_t)el < nenv;
  if (mine) {
    ObsEnvWords<C, EB> ew;
    obs_words_issue<C, EB>(ew, RecWords{S.words[el]}, part, a.na);
    obs_image_agents<C, EB>(O, ew, el, part, a.na);
  }
  __syncthreads();
  if (mine) obs_image_requests<C, EB>(O, el, part);
  __syncthreads();

  if (side == 0 && a.n && (uint32_t)tid < nenv) a.n[e0 + tid] = S.ix[tid] < 0 ? -1 : (int32_t)O.img[tid][0];
  if (uint32_t* sp = a.state[side]) {   // plane-major copy [words, M]: consecutive lanes, consecutive samples
    const SmallDiv by_env(nenv);
    for (uint32_t j = tid; j < total; j += BT) {
      const uint32_t w = by_env(j), e = j - w * nenv;
      sp[(int64_t)w * a.M + e0 + e] = S.words[e][w];
    }
  }
  const uint32_t per_env = na * L;
  if (uint4* xf = a.xfrag[side])   // the group's rows are whole 32-row tiles (EB * na % 32 == 0, checked on the host)
    stream_frags<BT, L, ObsLds<C, EB>::IMG>(O.lim, O.src[0], O.src[1], &O.img[0][0], xf, e0, nenv, a.na, tid);
  float* obs = a.obs[side];
  if (!obs) return;
  float* out = obs + e0 * per_env;
  if (a.quads)   // per_env % 4 == 0 and the rows 16-byte aligned (checked on the host); the plain writer
    stream_rows<BT, ObsLds<C, EB>::IMG, rows_nt<C>()>(O.lim, O.src[0], O.src[1], &O.img[0][0],
                                                      reinterpret_cast<f32x4*>(out), nenv, per_env >> 2, tid);
  else
    stream_rows_scalar<C, EB>(O, out, nenv, per_env, tid);
}
