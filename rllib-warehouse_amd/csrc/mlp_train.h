// mlp_train.h -- the policy / Q network's training forward and backward in exact f32 (wh_mlp_train_forward,
// wh_mlp_backward; include/warehouse_amd.h, MLP TRAINING).  Part of policy_mlp.hip's anonymous namespace;
// needs mlp_common.h (f32x16) and mlp_f32.h (mfma_f32) before it.
//
// Everything here is one tiled product C[M, N] = sum_k A(m, k) B(k, n) on v_mfma_f32_32x32x2_f32 (per
// output an f32 fma chain in ascending k), instantiated for the four operand layouts the six products
// of a three-layer ReLU MLP need, each reading the learner's own nn.Linear tensors and row-major
// activations as they lie in memory -- no packed blob, no transposed copy:
//
//   forward   H[r, j]  = act(sum_k X[r, k] W[j, k] + b[j])    A = X, B = W, both K-contiguous
//   dH        dH[r, k] = [h[r, k] > 0] sum_j dY[r, j] W[j, k]  A = dY K-contiguous, B = W N-contiguous
//   gW, gb    gW[j, k] = sum_r dY[r, j] X[r, k]                A = dY M-contiguous, B = X N-contiguous
//             gb[j]    = sum_r dY[r, j]                         = column N of the same product, B(r, N) = 1
//
// A workgroup of four waves walks K in chunks: every thread fetches its 8 + 8 elements of the next chunk
// into registers (lanes along the operand's contiguous dimension, so a wave's load is whole cache
// lines) while the MFMAs of the current chunk run from LDS, where both operands lie k-major (a wave's
// operand read is 32 consecutive words).  Two geometries (struct Wide, struct Deep), chosen by `rows`
// alone:
//   Wide  a 64 x 64 tile of C, one 32 x 32 accumulator per wave, K chunks of 32 (16 MFMAs per wave and
//         chunk): the fewest operand bytes per MFMA.  Above DEEP_MAX_ROWS rows.
//   Deep  a 32 x 32 tile of C shared by the four waves, K chunks of 64 of which wave w takes k-steps
//         8 w .. 8 w + 7; at the end waves 1-3 hand their accumulators over through LDS and wave 0 adds
//         them in wave order.  Four times the workgroups, each a quarter as many MFMAs deep: a batch of
//         a few hundred rows is bound by the depth of its MFMA chains (64 cycles each), not by bytes.
// Ragged edges -- rows, in_dim 37 / 82 / 145, the 9-wide logit side -- are predicated in the fetch: an
// element outside its tensor is never read and enters as an exact 0.0f.
//
// The bias gradient rides along as the all-ones column N of B (layout above): it is summed by the same
// MFMA chain in the same order as its weight gradients, and costs no pass of its own.
//
// Determinism.  No atomics.  An output element belongs to one wave (Wide), which adds its K range in
// ascending order, or to one workgroup (Deep), whose four waves each add their share of every chunk in
// ascending order before wave 0 adds the four sums in wave order.  A weight gradient reduces over
// K = rows; above SPLIT_ROWS rows that range is cut into ksplit(rows) slices (a function of rows alone)
// whose partial tiles go to `work`, and k_train_reduce adds them in ascending slice order.  So every
// value is a function of the inputs and of rows only.

namespace train {

constexpr int THREADS = 256;
struct Wide { static constexpr int T = 64, TK = 32; };   // workgroup tile T x T of C, K chunk
struct Deep { static constexpr int T = 32, TK = 64; };
constexpr int PER_THREAD = 8;              // elements of each operand per thread and chunk: T * TK / THREADS
constexpr int LDS_WORDS = 64 * 33;         // one operand's chunk, k-major with a pitch of T + 1 words
static_assert(Wide::T * Wide::TK == PER_THREAD * THREADS && Deep::T * Deep::TK == PER_THREAD * THREADS, "chunk");
static_assert(Wide::TK * (Wide::T + 1) <= LDS_WORDS && Deep::TK * (Deep::T + 1) <= LDS_WORDS, "LDS");
static_assert(3 * 16 * 64 <= 2 * LDS_WORDS, "Deep: three waves' accumulators fit the two operand buffers");
constexpr int64_t DEEP_MAX_ROWS = 1024;    // the Deep geometry up to this many rows
constexpr int64_t SPLIT_ROWS = 512;        // rows per K slice of a weight gradient
constexpr int MAX_SPLIT = 16;

enum Kind { FWD_RELU, FWD_LINEAR, DH, GRAD };

// One product.  `blocks` = ksplit * ceil(M / T) * ceil(NT / T) workgroups, NT = N + 1 for GRAD.
struct Job {
  const float* a;
  const float* b;
  float* c;            // FWD, DH: [M, N].  GRAD: gW [M, N], or with ksplit > 1 the partials [ksplit][M][N + 1]
  const float* aux;    // FWD: bias [N].  DH: the layer's activations h [M, N] (the mask h > 0)
  float* gb;           // GRAD with ksplit == 1: the bias gradient [M]
  int64_t M, N, K, lda, ldb;
  int64_t kslice;      // K range of one slice (a multiple of 64; K itself when ksplit == 1)
  uint32_t nbn, nbm, ksplit, blocks;
};

__host__ __device__ inline int64_t ksplit_of(int64_t rows) {
  const int64_t s = (rows + SPLIT_ROWS - 1) / SPLIT_ROWS;
  return s < 1 ? 1 : s > MAX_SPLIT ? MAX_SPLIT : s;
}

// Element (r, k) of an operand: CONTIG_K p[r * ld + k], else p[k * ld + r].  The thread's 8 elements
// of the chunk at k0, rows r0 .. r0 + T - 1; lanes run along the contiguous dimension.  ONES: row R of the
// operand (one past its last) is all ones (the bias-gradient column).
template <class G, bool CONTIG_K, bool ONES>
__device__ __forceinline__ void fetch(float (&v)[PER_THREAD], const float* __restrict__ p, int64_t ld, int64_t r0,
                                      int64_t R, int64_t k0, int64_t k1, int tid) {
#pragma unroll
  for (int q = 0; q < PER_THREAD; ++q) {
    const int idx = tid + THREADS * q;
    const int r = CONTIG_K ? idx / G::TK : idx % G::T;
    const int k = CONTIG_K ? idx % G::TK : idx / G::T;
    const int64_t gr = r0 + r, gk = k0 + k;
    float x = 0.0f;
    if (gk < k1) {
      if (gr < R) x = CONTIG_K ? p[gr * ld + gk] : p[gk * ld + gr];
      else if (ONES && gr == R) x = 1.0f;
    }
    v[q] = x;
  }
}

template <class G, bool CONTIG_K>
__device__ __forceinline__ void stage(float* lds, const float (&v)[PER_THREAD], int tid) {
#pragma unroll
  for (int q = 0; q < PER_THREAD; ++q) {
    const int idx = tid + THREADS * q;
    const int r = CONTIG_K ? idx / G::TK : idx % G::T;
    const int k = CONTIG_K ? idx % G::TK : idx / G::T;
    lds[k * (G::T + 1) + r] = v[q];
  }
}

template <Kind KIND, class G>
__device__ __forceinline__ void tile(const Job& j, uint32_t bid, float* lds_a, float* lds_b) {
  constexpr bool A_K = KIND != GRAD;                       // A K-contiguous
  constexpr bool B_K = KIND == FWD_RELU || KIND == FWD_LINEAR;   // B K-contiguous
  constexpr bool ONES = KIND == GRAD;
  constexpr bool DEEP = G::T == 32;
  constexpr int LD = G::T + 1;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int wm = DEEP ? 0 : w >> 1, wn = DEEP ? 0 : w & 1;   // the wave's 32 x 32 tile within the workgroup's
  const int ks = DEEP ? 16 * w : 0;                          // ... and its first k of every chunk
  const uint32_t per = j.nbm * j.nbn;
  const uint32_t slice = bid / per, t = bid % per;
  const int64_t m0 = (int64_t)(t / j.nbn) * G::T, n0 = (int64_t)(t % j.nbn) * G::T;
  const int64_t NT = j.N + (ONES ? 1 : 0);
  const int64_t k0 = (int64_t)slice * j.kslice;
  const int64_t k1 = k0 + j.kslice < j.K ? k0 + j.kslice : j.K;
  // Wide: a wave whose 32 x 32 tile lies wholly outside C only helps to stage
  const bool active = m0 + 32 * wm < j.M && n0 + 32 * wn < NT;
  f32x16 acc{};
  float va[PER_THREAD], vb[PER_THREAD];
  if (k0 < k1) {
    fetch<G, A_K, false>(va, j.a, j.lda, m0, j.M, k0, k1, tid);
    fetch<G, B_K, ONES>(vb, j.b, j.ldb, n0, j.N, k0, k1, tid);
  }
  for (int64_t kc = k0; kc < k1; kc += G::TK) {
    stage<G, A_K>(lds_a, va, tid);
    stage<G, B_K>(lds_b, vb, tid);
    __syncthreads();
    if (kc + G::TK < k1) {
      fetch<G, A_K, false>(va, j.a, j.lda, m0, j.M, kc + G::TK, k1, tid);
      fetch<G, B_K, ONES>(vb, j.b, j.ldb, n0, j.N, kc + G::TK, k1, tid);
    }
    if (active) {
#pragma unroll
      for (int s = 0; s < (DEEP ? 8 : 16); ++s)
        acc = mfma_f32(lds_a[(ks + 2 * s + h) * LD + 32 * wm + i], lds_b[(ks + 2 * s + h) * LD + 32 * wn + i], acc);
    }
    __syncthreads();
  }
  if (DEEP) {
    // (every wave of the workgroup arrives here: `active` holds for all four or for none, and nothing
    // above returns.)  The operand buffers are free after the loop's last barrier: waves 1-3 park their
    // accumulators there, register g of lane l at word (16 (w - 1) + g) 64 + l of one buffer or the other
    if (w > 0) {
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int word = (16 * (w - 1) + g) * 64 + lane;
        *(word < LDS_WORDS ? lds_a + word : lds_b + (word - LDS_WORDS)) = acc[g];
      }
    }
    __syncthreads();
    if (w > 0) return;
#pragma unroll
    for (int v = 1; v < 4; ++v)
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int word = (16 * (v - 1) + g) * 64 + lane;
        acc[g] += *(word < LDS_WORDS ? lds_a + word : lds_b + (word - LDS_WORDS));
      }
  }
  if (!active) return;
  // register g of the accumulator: row (g & 3) + 8 (g >> 2) + 4 h of the wave's tile, column i
  const int64_t n = n0 + 32 * wn + i;
  if (n >= NT) return;
  float bias = 0.0f;
  if (KIND == FWD_RELU || KIND == FWD_LINEAR) bias = j.aux[n];
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int64_t m = m0 + 32 * wm + (g & 3) + 8 * (g >> 2) + 4 * h;
    if (m >= j.M) continue;
    float v = acc[g];
    if (KIND == FWD_RELU) v = fmaxf(v + bias, 0.0f);
    if (KIND == FWD_LINEAR) v = v + bias;
    if (KIND == DH) v = j.aux[m * j.N + n] > 0.0f ? v : 0.0f;
    if (KIND == GRAD) {
      if (j.ksplit > 1) j.c[((int64_t)slice * j.M + m) * NT + n] = v;
      else if (n < j.N) j.c[m * j.N + n] = v;
      else j.gb[m] = v;
    } else {
      j.c[m * j.N + n] = v;
    }
  }
}

template <Kind KIND, class G>
__global__ __launch_bounds__(THREADS) void k_train(Job j) {
  __shared__ float lds_a[LDS_WORDS], lds_b[LDS_WORDS];
  tile<KIND, G>(j, blockIdx.x, lds_a, lds_b);
}

// Two products with no dependency between them in one launch: workgroups 0 .. g.blocks - 1 are the weight
// gradient's, the rest dH's (the job is workgroup-uniform).
template <class G>
__global__ __launch_bounds__(THREADS) void k_train_pair(Job g, Job d) {
  __shared__ float lds_a[LDS_WORDS], lds_b[LDS_WORDS];
  if (blockIdx.x < g.blocks) tile<GRAD, G>(g, blockIdx.x, lds_a, lds_b);
  else tile<DH, G>(d, blockIdx.x - g.blocks, lds_a, lds_b);
}

// The second pass of the split weight gradients: element e of gradient q is the sum of its ksplit
// partials in ascending slice order; column N of a partial row is the bias gradient.
struct Reduce {
  const float* part[3];
  float* gw[3];
  float* gb[3];
  int64_t M[3], N[3];
  int64_t first[4];    // first[q]: the first flat element of gradient q; first[3]: all of them
  int32_t ksplit;
};

__global__ __launch_bounds__(THREADS) void k_train_reduce(Reduce r) {
  const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (e >= r.first[3]) return;
  const int q = e >= r.first[2] ? 2 : e >= r.first[1] ? 1 : 0;
  const int64_t o = e - r.first[q], NT = r.N[q] + 1, size = r.M[q] * NT;
  float s = r.part[q][o];
  for (int k = 1; k < r.ksplit; ++k) s += r.part[q][k * size + o];
  const int64_t m = o / NT, n = o % NT;
  if (n < r.N[q]) r.gw[q][m * r.N[q] + n] = s;
  else r.gb[q][m] = s;
}

// ------------------------------------------------------------- several networks of one shape in one launch
// wh_mlp_train_forward_multi / wh_mlp_backward_multi: the same product of up to MAX_NETS networks side by
// side in one grid.  All networks share the geometry (`shape`: one M, N, K, ksplit and block count) and
// differ in their five pointers only, so the argument carries the geometry once.  Workgroups
// net * shape.blocks .. (net + 1) * shape.blocks - 1 are network net's; the index depends on blockIdx.x and
// the argument only, so it is workgroup-uniform and the network's pointers are scalar loads from the
// argument segment (no register array is indexed).  The workgroup then runs tile<KIND, G> on the Job a
// single-network launch would have been given and with the block id it would have had: tile is a
// function of those two alone, so every output is byte for byte the single-network launch's.
constexpr int MAX_NETS = 4;

struct NetPtrs {
  const float* a;
  const float* b;
  float* c;
  const float* aux;
  float* gb;
};

struct MultiJob {
  Job shape;              // the geometry of every network's product; its own five pointers are unused
  NetPtrs net[MAX_NETS];
  uint32_t nnets;
};

__device__ __forceinline__ Job job_of(const MultiJob& m, uint32_t net) {
  const NetPtrs p = m.net[__builtin_amdgcn_readfirstlane(net)];
  Job j = m.shape;
  j.a = p.a; j.b = p.b; j.c = p.c; j.aux = p.aux; j.gb = p.gb;
  return j;
}

// one product of every network: a forward layer, or the last weight gradient
template <Kind KIND, class G>
__global__ __launch_bounds__(THREADS) void k_train_multi(MultiJob m) {
  __shared__ float lds_a[LDS_WORDS], lds_b[LDS_WORDS];
  const uint32_t per = m.shape.blocks;
  tile<KIND, G>(job_of(m, blockIdx.x / per), blockIdx.x % per, lds_a, lds_b);
}

// k_train_pair for every network: all the weight gradients' workgroups first (the deeper product), then
// all the dH's
template <class G>
__global__ __launch_bounds__(THREADS) void k_train_pair_multi(MultiJob g, MultiJob d) {
  __shared__ float lds_a[LDS_WORDS], lds_b[LDS_WORDS];
  const uint32_t grad_blocks = g.nnets * g.shape.blocks;
  if (blockIdx.x < grad_blocks) {
    const uint32_t per = g.shape.blocks;
    tile<GRAD, G>(job_of(g, blockIdx.x / per), blockIdx.x % per, lds_a, lds_b);
  } else {
    const uint32_t b = blockIdx.x - grad_blocks, per = d.shape.blocks;
    tile<DH, G>(job_of(d, b / per), b % per, lds_a, lds_b);
  }
}

// k_train_reduce over the three gradients of every network (up to 12): workgroups net * per ..
// (net + 1) * per - 1, per = ceil(first[3] / THREADS), are network net's and walk its elements as
// k_train_reduce's do.
struct ReducePtrs {
  const float* part[3];
  float* gw[3];
  float* gb[3];
};

struct ReduceMulti {
  int64_t M[3], N[3];
  int64_t first[4];
  int32_t ksplit;
  uint32_t per;           // workgroups per network
  ReducePtrs net[MAX_NETS];
};

__global__ __launch_bounds__(THREADS) void k_train_reduce_multi(ReduceMulti r) {
  const uint32_t net = __builtin_amdgcn_readfirstlane(blockIdx.x / r.per);
  const int64_t e = (int64_t)(blockIdx.x % r.per) * THREADS + threadIdx.x;
  if (e >= r.first[3]) return;
  const ReducePtrs p = r.net[net];
  // (the gradient index differs from thread to thread: selected by comparison, not by indexing)
  const bool q2 = e >= r.first[2], q1 = e >= r.first[1];
  const float* part = q2 ? p.part[2] : q1 ? p.part[1] : p.part[0];
  float* gw = q2 ? p.gw[2] : q1 ? p.gw[1] : p.gw[0];
  float* gb = q2 ? p.gb[2] : q1 ? p.gb[1] : p.gb[0];
  const int64_t M = q2 ? r.M[2] : q1 ? r.M[1] : r.M[0], N = q2 ? r.N[2] : q1 ? r.N[1] : r.N[0];
  const int64_t o = e - (q2 ? r.first[2] : q1 ? r.first[1] : r.first[0]), NT = N + 1, size = M * NT;
  float s = part[o];
  for (int k = 1; k < r.ksplit; ++k) s += part[k * size + o];
  const int64_t m = o / NT, n = o % NT;
  if (n < N) gw[m * N + n] = s;
  else gb[m] = s;
}

// ------------------------------------------------------------------------------------------ host side
struct Dims { int64_t in, h0, h1; };

// floats of one slice of all three weight gradients' partial tiles ([M][N + 1] each)
inline int64_t partial_floats(const Dims& d) { return 9 * (d.h1 + 1) + d.h1 * (d.h0 + 1) + d.h0 * (d.in + 1); }

// `work`: dH1 [rows, h1], dH0 [rows, h0], then -- above SPLIT_ROWS rows -- ksplit slices of partials
inline int64_t work_bytes(const Dims& d, int64_t rows) {
  const int64_t s = ksplit_of(rows);
  const int64_t f = rows * (d.h0 + d.h1) + (s > 1 ? s * partial_floats(d) : 0);
  return f > 0 ? (4 * f + 15) / 16 * 16 : 16;
}

inline uint32_t cdiv(int64_t a, int64_t b) { return (uint32_t)((a + b - 1) / b); }

inline bool deep(int64_t rows) { return rows <= DEEP_MAX_ROWS; }

inline Job make_job(int T, Kind kind, const float* a, int64_t lda, const float* b, int64_t ldb, float* c, const float* aux,
                    float* gb, int64_t M, int64_t N, int64_t K, int64_t ksplit) {
  Job j{};
  j.a = a; j.b = b; j.c = c; j.aux = aux; j.gb = gb;
  j.M = M; j.N = N; j.K = K; j.lda = lda; j.ldb = ldb;
  j.ksplit = (uint32_t)ksplit;
  j.kslice = ksplit > 1 ? ((K + ksplit - 1) / ksplit + 63) / 64 * 64 : K;
  j.nbm = cdiv(M, T);
  j.nbn = cdiv(N + (kind == GRAD ? 1 : 0), T);
  j.blocks = j.ksplit * j.nbm * j.nbn;
  return j;
}

template <Kind KIND, class G>
inline void launch(const Job& j, hipStream_t s) {
  if (j.blocks) hipLaunchKernelGGL((k_train<KIND, G>), dim3(j.blocks), dim3(THREADS), 0, s, j);
}

template <class G>
inline int forward_on(const Dims& d, const wh_mlp_weights& w, int64_t rows, const float* obs, float* h0, float* h1,
                      float* logits, hipStream_t s) {
  constexpr int T = G::T;
  launch<FWD_RELU, G>(make_job(T, FWD_RELU, obs, d.in, w.w0, d.in, h0, w.b0, nullptr, rows, d.h0, d.in, 1), s);
  launch<FWD_RELU, G>(make_job(T, FWD_RELU, h0, d.h0, w.w1, d.h0, h1, w.b1, nullptr, rows, d.h1, d.h0, 1), s);
  launch<FWD_LINEAR, G>(make_job(T, FWD_LINEAR, h1, d.h1, w.w2, d.h1, logits, w.b2, nullptr, rows, 9, d.h1, 1), s);
  return hip_rc(hipGetLastError());
}

inline int forward(const Dims& d, const wh_mlp_weights& w, int64_t rows, const float* obs, float* h0, float* h1,
                   float* logits, hipStream_t s) {
  return deep(rows) ? forward_on<Deep>(d, w, rows, obs, h0, h1, logits, s)
                    : forward_on<Wide>(d, w, rows, obs, h0, h1, logits, s);
}

template <class G>
inline int backward_on(const Dims& d, const wh_mlp_weights& w, int64_t rows, const float* obs, const float* h0,
                       const float* h1, const float* dz, const wh_mlp_grads& g, void* work, hipStream_t s) {
  constexpr int T = G::T;
  float* dh1 = static_cast<float*>(work);
  float* dh0 = dh1 + rows * d.h1;
  float* part = dh0 + rows * d.h0;
  const int64_t ks = ksplit_of(rows);
  const int64_t p2 = 9 * (d.h1 + 1), p1 = d.h1 * (d.h0 + 1), p0 = d.h0 * (d.in + 1);
  float* part2 = part;
  float* part1 = part2 + ks * p2;
  float* part0 = part1 + ks * p1;
  const bool split = ks > 1;
  // dH1 = (dZ W2) . [h1 > 0]   beside   gW2 = dZ^T h1, gb2
  const Job g2 = make_job(T, GRAD, dz, 9, h1, d.h1, split ? part2 : g.w2, nullptr, g.b2, 9, d.h1, rows, ks);
  const Job d1 = make_job(T, DH, dz, 9, w.w2, d.h1, dh1, h1, nullptr, rows, d.h1, 9, 1);
  hipLaunchKernelGGL(k_train_pair<G>, dim3(g2.blocks + d1.blocks), dim3(THREADS), 0, s, g2, d1);
  // dH0 = (dH1 W1) . [h0 > 0]   beside   gW1 = dH1^T h0, gb1
  const Job g1 = make_job(T, GRAD, dh1, d.h1, h0, d.h0, split ? part1 : g.w1, nullptr, g.b1, d.h1, d.h0, rows, ks);
  const Job d0 = make_job(T, DH, dh1, d.h1, w.w1, d.h0, dh0, h0, nullptr, rows, d.h0, d.h1, 1);
  hipLaunchKernelGGL(k_train_pair<G>, dim3(g1.blocks + d0.blocks), dim3(THREADS), 0, s, g1, d0);
  // gW0 = dH0^T x, gb0
  launch<GRAD, G>(make_job(T, GRAD, dh0, d.h0, obs, d.in, split ? part0 : g.w0, nullptr, g.b0, d.h0, d.in, rows, ks), s);
  if (split) {
    Reduce r{};
    const float* parts[3] = {part2, part1, part0};
    float* gw[3] = {g.w2, g.w1, g.w0};
    float* gb[3] = {g.b2, g.b1, g.b0};
    const int64_t M[3] = {9, d.h1, d.h0}, N[3] = {d.h1, d.h0, d.in}, P[3] = {p2, p1, p0};
    for (int q = 0; q < 3; ++q) {
      r.part[q] = parts[q]; r.gw[q] = gw[q]; r.gb[q] = gb[q];
      r.M[q] = M[q]; r.N[q] = N[q];
      r.first[q + 1] = r.first[q] + P[q];
    }
    r.ksplit = (int32_t)ks;
    hipLaunchKernelGGL(k_train_reduce, dim3(cdiv(r.first[3], THREADS)), dim3(THREADS), 0, s, r);
  }
  return hip_rc(hipGetLastError());
}

inline int backward(const Dims& d, const wh_mlp_weights& w, int64_t rows, const float* obs, const float* h0,
                    const float* h1, const float* dz, const wh_mlp_grads& g, void* work, hipStream_t s) {
  return deep(rows) ? backward_on<Deep>(d, w, rows, obs, h0, h1, dz, g, work, s)
                    : backward_on<Wide>(d, w, rows, obs, h0, h1, dz, g, work, s);
}

// ---- several networks (wh_mlp_train_forward_multi, wh_mlp_backward_multi).  Every MultiJob is the Job
// forward_on / backward_on make for one network (make_job with that network's pointers), the geometry
// kept once.
static_assert(MAX_NETS == WH_MLP_TRAIN_MAX_NETS, "mlp_train.h and the header agree on the network limit");

// network i's slices of `work`, as backward_on lays them out
struct Work {
  float *dh1, *dh0, *part2, *part1, *part0;
};

inline Work work_of(const Dims& d, int64_t rows, void* work) {
  const int64_t ks = ksplit_of(rows);
  Work w;
  w.dh1 = static_cast<float*>(work);
  w.dh0 = w.dh1 + rows * d.h1;
  w.part2 = w.dh0 + rows * d.h0;
  w.part1 = w.part2 + ks * 9 * (d.h1 + 1);
  w.part0 = w.part1 + ks * d.h1 * (d.h0 + 1);
  return w;
}

inline MultiJob make_multi(int T, Kind kind, int n, const NetPtrs* p, int64_t lda, int64_t ldb, int64_t M, int64_t N,
                           int64_t K, int64_t ksplit) {
  MultiJob m{};
  m.shape = make_job(T, kind, nullptr, lda, nullptr, ldb, nullptr, nullptr, nullptr, M, N, K, ksplit);
  for (int i = 0; i < n; ++i) m.net[i] = p[i];
  m.nnets = (uint32_t)n;
  return m;
}

template <Kind KIND, class G>
inline void launch_multi(const MultiJob& m, hipStream_t s) {
  if (m.nnets * m.shape.blocks)
    hipLaunchKernelGGL((k_train_multi<KIND, G>), dim3(m.nnets * m.shape.blocks), dim3(THREADS), 0, s, m);
}

template <class G>
inline int forward_multi_on(const Dims& d, int n, const wh_mlp_train_job* jobs, int64_t rows, hipStream_t s) {
  constexpr int T = G::T;
  NetPtrs p[MAX_NETS];
  for (int i = 0; i < n; ++i) p[i] = NetPtrs{jobs[i].obs, jobs[i].w.w0, jobs[i].h0, jobs[i].w.b0, nullptr};
  launch_multi<FWD_RELU, G>(make_multi(T, FWD_RELU, n, p, d.in, d.in, rows, d.h0, d.in, 1), s);
  for (int i = 0; i < n; ++i) p[i] = NetPtrs{jobs[i].h0, jobs[i].w.w1, jobs[i].h1, jobs[i].w.b1, nullptr};
  launch_multi<FWD_RELU, G>(make_multi(T, FWD_RELU, n, p, d.h0, d.h0, rows, d.h1, d.h0, 1), s);
  for (int i = 0; i < n; ++i) p[i] = NetPtrs{jobs[i].h1, jobs[i].w.w2, jobs[i].logits, jobs[i].w.b2, nullptr};
  launch_multi<FWD_LINEAR, G>(make_multi(T, FWD_LINEAR, n, p, d.h1, d.h1, rows, 9, d.h1, 1), s);
  return hip_rc(hipGetLastError());
}

inline int forward_multi(const Dims& d, int n, const wh_mlp_train_job* jobs, int64_t rows, hipStream_t s) {
  return deep(rows) ? forward_multi_on<Deep>(d, n, jobs, rows, s) : forward_multi_on<Wide>(d, n, jobs, rows, s);
}

template <class G>
inline int backward_multi_on(const Dims& d, int n, const wh_mlp_train_job* jobs, int64_t rows, hipStream_t s) {
  constexpr int T = G::T;
  const int64_t ks = ksplit_of(rows);
  const bool split = ks > 1;
  Work wk[MAX_NETS];
  NetPtrs pg[MAX_NETS], pd[MAX_NETS];
  for (int i = 0; i < n; ++i) wk[i] = work_of(d, rows, jobs[i].work);
  // dH1 beside gW2, gb2
  for (int i = 0; i < n; ++i) {
    const wh_mlp_train_job& j = jobs[i];
    pg[i] = NetPtrs{j.dlogits, j.h1, split ? wk[i].part2 : j.g.w2, nullptr, j.g.b2};
    pd[i] = NetPtrs{j.dlogits, j.w.w2, wk[i].dh1, j.h1, nullptr};
  }
  const MultiJob g2 = make_multi(T, GRAD, n, pg, 9, d.h1, 9, d.h1, rows, ks);
  const MultiJob d1 = make_multi(T, DH, n, pd, 9, d.h1, rows, d.h1, 9, 1);
  hipLaunchKernelGGL(k_train_pair_multi<G>, dim3(n * (g2.shape.blocks + d1.shape.blocks)), dim3(THREADS), 0, s, g2, d1);
  // dH0 beside gW1, gb1
  for (int i = 0; i < n; ++i) {
    const wh_mlp_train_job& j = jobs[i];
    pg[i] = NetPtrs{wk[i].dh1, j.h0, split ? wk[i].part1 : j.g.w1, nullptr, j.g.b1};
    pd[i] = NetPtrs{wk[i].dh1, j.w.w1, wk[i].dh0, j.h0, nullptr};
  }
  const MultiJob g1 = make_multi(T, GRAD, n, pg, d.h1, d.h0, d.h1, d.h0, rows, ks);
  const MultiJob d0 = make_multi(T, DH, n, pd, d.h1, d.h0, rows, d.h0, d.h1, 1);
  hipLaunchKernelGGL(k_train_pair_multi<G>, dim3(n * (g1.shape.blocks + d0.shape.blocks)), dim3(THREADS), 0, s, g1, d0);
  // gW0, gb0
  for (int i = 0; i < n; ++i) {
    const wh_mlp_train_job& j = jobs[i];
    pg[i] = NetPtrs{wk[i].dh0, j.obs, split ? wk[i].part0 : j.g.w0, nullptr, j.g.b0};
  }
  launch_multi<GRAD, G>(make_multi(T, GRAD, n, pg, d.h0, d.in, d.h0, d.in, rows, ks), s);
  if (split) {
    ReduceMulti r{};
    const int64_t M[3] = {9, d.h1, d.h0}, N[3] = {d.h1, d.h0, d.in};
    for (int q = 0; q < 3; ++q) {
      r.M[q] = M[q]; r.N[q] = N[q];
      r.first[q + 1] = r.first[q] + M[q] * (N[q] + 1);
    }
    r.ksplit = (int32_t)ks;
    r.per = cdiv(r.first[3], THREADS);
    for (int i = 0; i < n; ++i) {
      const wh_mlp_grads& g = jobs[i].g;
      r.net[i] = ReducePtrs{{wk[i].part2, wk[i].part1, wk[i].part0}, {g.w2, g.w1, g.w0}, {g.b2, g.b1, g.b0}};
    }
    hipLaunchKernelGGL(k_train_reduce_multi, dim3(n * r.per), dim3(THREADS), 0, s, r);
  }
  return hip_rc(hipGetLastError());
}

inline int backward_multi(const Dims& d, int n, const wh_mlp_train_job* jobs, int64_t rows, hipStream_t s) {
  return deep(rows) ? backward_multi_on<Deep>(d, n, jobs, rows, s) : backward_multi_on<Wide>(d, n, jobs, rows, s);
}

}  // namespace train
