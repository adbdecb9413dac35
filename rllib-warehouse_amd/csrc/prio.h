// prio.h -- the replay priority tree's three kernels (include/warehouse_amd.h, REPLAY PRIORITIES).
// Included by warehouse_amd.hip inside its namespace, after replay.h; the row-scoped DPP moves are
// step_wide.h's (row_ror, row_or, row_or64).
//
// A radix-16 sum tree in integers: leaves are uint32 fixed-point priorities, every level above them
// uint64 sums, the 16 children of an entry one 128-byte line.  All arithmetic is integer and every
// update is a commutative, exact 64-bit add (or a u32 exchange / max on a leaf), so the tree a
// sequence of calls leaves does not depend on the order lanes, waves or workgroups ran in, and is
// the host engine's bit for bit.

constexpr uint32_t PUR_PRIO = 7;
constexpr int PRIO_LV = wh_abi::PRIO_MAX_LEVELS;

struct PrioTree {   // wh_replay_prio with its shape (wh_abi::PrioShape)
  uint32_t* leaf;
  uint64_t* node;
  uint32_t* max_q;
  int64_t count;
  int32_t levels;
  int64_t n[PRIO_LV + 1];     // entries of level k (n[0] = count)
  int64_t off[PRIO_LV + 1];   // first word of level k >= 1 in `node`
};

__device__ __forceinline__ unsigned long long* prio_entry(const PrioTree& t, int k, int64_t j) {
  return reinterpret_cast<unsigned long long*>(t.node + t.off[k] + j);
}

// the row shifted right by N lanes, zeros shifted in (full-rate DPP move)
template <int N>
__device__ __forceinline__ uint32_t row_shr(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + N, 0xF, 0xF, true);
}
template <int N>
__device__ __forceinline__ uint64_t row_shr64(uint64_t v) {
  return ((uint64_t)row_shr<N>((uint32_t)(v >> 32)) << 32) | row_shr<N>((uint32_t)v);
}
template <int N>
__device__ __forceinline__ uint64_t row_ror64(uint64_t v) {
  return ((uint64_t)row_ror<N>((uint32_t)(v >> 32)) << 32) | row_ror<N>((uint32_t)v);
}
// inclusive prefix sums over the 16 lanes of the row
__device__ __forceinline__ uint64_t row_scan64(uint64_t v) {
  v += row_shr64<1>(v);
  v += row_shr64<2>(v);
  v += row_shr64<4>(v);
  v += row_shr64<8>(v);
  return v;
}
// the row's (wrapping) sum, in every lane
__device__ __forceinline__ uint64_t row_sum64(uint64_t v) {
  v += row_ror64<8>(v);
  v += row_ror64<4>(v);
  v += row_ror64<2>(v);
  v += row_ror64<1>(v);
  return v;
}

// ----------------------------------------------------------------------------- sample
struct PrioSampleParams {
  PrioTree t;
  int64_t M;
  const uint64_t* u;        // [M] injected draws, or null (philox, purpose 7)
  uint32_t k0, k1, d0, d1;  // seed and draw, low / high words
  int64_t* idx_out;
  uint32_t* q_out;
  uint64_t* total_out;
};

// One DPP row per sample, four samples per wave.  Per level lane j loads child j of the entry the
// descent stands on (one line per row), an inclusive row scan gives the prefix sums, the row's slice
// of a ballot the first child whose prefix exceeds the mass, and a masked row OR that child's
// exclusive prefix.  A row past M shadows sample M - 1 and writes nothing: all 64 lanes stay
// converged through every cross-lane operation.  The descent cannot leave the tree whatever the
// buffers hold: a child index is below 16 and the entry index is clamped to its level.
__global__ __launch_bounds__(BT) void k_prio_sample(PrioSampleParams a) {
  const PrioTree& t = a.t;
  const uint32_t tid = threadIdx.x, lane = tid & 15u;
  const int64_t row = (int64_t)blockIdx.x * (BT / 16) + (tid >> 4);
  const bool live = row < a.M;
  const int64_t m = live ? row : a.M - 1;
  const int K = t.levels;
  // the root and the level below it, before the draw
  const uint64_t total = t.node[t.off[K]];
  uint64_t v = K > 1 ? t.node[t.off[K - 1] + lane] : (uint64_t)t.leaf[lane];
  uint64_t r;
  if (a.u) {
    r = a.u[m];
  } else {
    const uint4 w = philox10(make_uint4((uint32_t)m, a.d0, a.d1, PUR_PRIO << 24), a.k0, a.k1);
    r = (uint64_t)w.x << 32 | w.y;
  }
  uint64_t mass = __umul64hi(r, total);
  int64_t pos = 0;   // the entry of level k + 1 whose children v holds
  uint32_t q = 0;
  for (int k = K - 1;; --k) {
    const uint64_t inc = row_scan64(v);
    const uint32_t bits = (uint32_t)(__ballot(inc > mass) >> (tid & 48u)) & 0xFFFFu;
    const uint32_t j = bits ? (uint32_t)__builtin_ctz(bits) : 15u;
    mass -= row_or64(lane == j ? inc - v : 0ull);
    pos = pos * 16 + j;
    if (pos >= t.n[k]) pos = t.n[k] - 1;   // (never in a tree whose sums and padding are right)
    if (k == 0) {
      q = row_or(lane == j ? (uint32_t)v : 0u);
      break;
    }
    v = k > 1 ? t.node[t.off[k - 1] + pos * 16 + lane] : (uint64_t)t.leaf[pos * 16 + lane];
  }
  if (live && lane == 0) {
    a.idx_out[m] = total ? pos : -1;
    if (a.q_out) a.q_out[m] = total ? q : 0u;
  }
  if (a.total_out && blockIdx.x == 0 && tid == 0) a.total_out[0] = total;
}

// ----------------------------------------------------------------------------- update
struct PrioUpdateParams {
  PrioTree t;
  int64_t M;
  const int64_t* idx;
  const float* p;
  int phase;   // 0: clear the touched leaves; 1: raise them to their q
};

// Lane = sample, run twice on the stream.  Phase 0 exchanges the leaf for 0 and takes what was there
// out of the ancestors (of duplicates one lane finds the old value, the others 0); phase 1 raises
// the leaf to q with a max and adds what the max gained: the gains of duplicates telescope to the
// largest q, whatever the order.  The scattered lower levels take one atomic per lane and level;
// the root and the level below it (at most 16 entries), which every lane would hit, take one
// atomic per workgroup and entry, reduced in LDS first.
__global__ __launch_bounds__(BT) void k_prio_update(PrioUpdateParams a) {
  __shared__ unsigned long long bin[17];   // the level under the root, then the root
  __shared__ uint32_t qmax;
  const PrioTree& t = a.t;
  const int tid = threadIdx.x, K = t.levels;
  if (tid < 17) bin[tid] = 0ull;
  if (tid == 17) qmax = 0u;
  __syncthreads();
  const int64_t m = (int64_t)blockIdx.x * BT + tid;
  int64_t ix = -1;
  if (m < a.M) {
    ix = a.idx[m];
    if (ix < 0 || ix >= t.count) ix = -1;
  }
  uint64_t delta = 0;
  if (ix >= 0) {
    if (a.phase == 0) {
      delta = 0ull - (uint64_t)atomicExch(&t.leaf[ix], 0u);
    } else {
      const uint32_t q = wh_abi::prio_quantise(a.p[m]);
      const uint32_t prev = atomicMax(&t.leaf[ix], q);
      if (q > prev) delta = (uint64_t)(q - prev);
      atomicMax(&qmax, q);
    }
  }
  if (delta) {
    for (int k = 1; k <= K - 2; ++k) atomicAdd(prio_entry(t, k, ix >> (4 * k)), (unsigned long long)delta);
    if (K >= 2) atomicAdd(&bin[ix >> (4 * (K - 1))], (unsigned long long)delta);
    atomicAdd(&bin[16], (unsigned long long)delta);
  }
  __syncthreads();
  if (tid < 16 && K >= 2 && bin[tid]) atomicAdd(prio_entry(t, K - 1, tid), bin[tid]);
  if (tid == 16 && bin[16]) atomicAdd(prio_entry(t, K, 0), bin[16]);
  if (tid == 17 && qmax) atomicMax(t.max_q, qmax);
}

// ----------------------------------------------------------------------------- fill
struct PrioFillParams {
  PrioTree t;
  int64_t first, end;   // leaves [first, end)
  int64_t base;         // first rounded down to a workgroup's 256 leaves
  int mode;
  uint32_t q;
};

// Lane = leaf: workgroup b owns leaves [base + 256 b, +256), which share every ancestor from level
// 2 up, and a row of 16 lanes owns one level-1 entry.  Plain leaf loads and stores (a fill is
// ordered against updates by the stream); one add of the row's summed delta to level 1, and one add
// of the workgroup's to each level above, issued by one lane per level.
__global__ __launch_bounds__(BT) void k_prio_fill(PrioFillParams a) {
  __shared__ uint64_t rows[BT / 16];
  const PrioTree& t = a.t;
  const int tid = threadIdx.x, K = t.levels;
  const int64_t wg0 = a.base + (int64_t)blockIdx.x * BT, i = wg0 + tid;
  const uint32_t q = a.mode ? *t.max_q : a.q;
  uint64_t d = 0;
  if (i >= a.first && i < a.end) {
    d = (uint64_t)q - (uint64_t)t.leaf[i];
    t.leaf[i] = q;
  }
  const uint64_t s = row_sum64(d);
  if ((tid & 15) == 0) {
    rows[tid >> 4] = s;
    if (s) atomicAdd(prio_entry(t, 1, i >> 4), (unsigned long long)s);
  }
  __syncthreads();
  const int k = tid + 2;
  if (k <= K) {
    uint64_t w = 0;
#pragma unroll
    for (int r = 0; r < BT / 16; ++r) w += rows[r];
    if (w) atomicAdd(prio_entry(t, k, wg0 >> (4 * k)), (unsigned long long)w);
  }
}
