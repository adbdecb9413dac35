// mlp_f32.h -- the policy network in exact f32 (k_mlp_f32, precision WH_MLP_F32).  Part of
// policy_mlp.hip's anonymous namespace; needs mlp_common.h before it.

// The same network in exact f32 (the reference policy is TF fp32): every layer on
// v_mfma_f32_32x32x2_f32, whose result is bit-for-bit a k-ordered f32 fmaf chain, so logits differ
// from a float32 reference only by summation order (~1e-7 relative).  Same orientation as the
// bf16 kernel: a wave's 32 samples are the tile COLUMNS, so a 32x32 f32 accumulator register g
// (rows (g&3) + 8(g>>2) + 4h on lane half h) is, after bias + ReLU, directly the B operand of one
// K = 2 step of the next layer -- the k pair (r_g, r_g + 4) is folded into the packed weights.
// Weights stream from L2 as one 256-byte A operand per MFMA, in exactly the order the MFMAs
// consume them, through a 16-deep register ring (a load issued 16 MFMAs = ~1,000 cycles ahead).
template <int IN_, int H0_, int H1_, int PASSES_>
struct NetF {
  static constexpr int IN = IN_, H0 = H0_, H1 = H1_, PASSES = PASSES_, OUT = 9;
  static constexpr int KS0 = (IN + 1) / 2;                 // layer-0 K = 2 steps
  static constexpr int KS0P = (KS0 + 15) / 16 * 16;        // padded so every segment is 16 ops long
  static constexpr int T0 = H0 / 32, T1 = H1 / 32, T1P = T1 / PASSES;
  static constexpr int RING = 16;
  // operand stream (64 f32 per op, lane-linear): per pass { per layer-0 tile t: W0 [KS0P],
  // W1 [16 g][T1P u] }, then W2 [T1P u][16 g]; RING zero ops of read-ahead padding; then f32
  // biases b0[H0], b1[H1], b2[32]
  static constexpr int64_t OPS = (int64_t)PASSES * (T0 * (KS0P + 16 * T1P) + 16 * T1P);
  static constexpr int64_t BIAS_OFF = (OPS + RING) * 256;
  static constexpr int64_t BYTES = BIAS_OFF + 4 * (H0 + H1 + 32);
  static_assert(H0 % 32 == 0 && H1 % 32 == 0 && T1 % PASSES == 0, "tile shapes");
};

__device__ __forceinline__ f32x16 mfma_f32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

template <class N, class G = GridOne>
__global__ __launch_bounds__(256) void k_mlp_f32(typename G::Params p) {
  const G grid(p);                      // whose workgroup this is (mlp_common.h, grid policies)
  const MlpArgs& a = grid.job(p);
  __shared__ float bias[N::H0 + N::H1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n = lane & 31, h = lane >> 5;
  const float* ops = static_cast<const float*>(a.packed);
  const float* gb = reinterpret_cast<const float*>(static_cast<const uint8_t*>(a.packed) + N::BIAS_OFF);
  for (int i = tid; i < N::H0 + N::H1; i += 256) bias[i] = gb[i];
  __syncthreads();
  const int64_t task = (int64_t)grid.bid() * 4 + w;
  const int64_t row0 = task * 32;
  if (row0 >= a.rows) return;
  const int64_t row = row0 + n;
  const bool live = row < a.rows;
  // X^T operands: lane (n, h) holds obs[row n][2s + h]
  float xop[N::KS0P];
  {
    const float* x = a.obs + (live ? row : row0) * N::IN;
#pragma unroll
    for (int q = 0; q < N::KS0P; ++q) {
      const int k = 2 * q + h;
      xop[q] = (k < N::IN && live) ? x[k < N::IN ? k : 0] : 0.0f;
    }
  }
  const float* sp = ops + lane;           // op i of this lane: sp[i * 64]
  float ring[N::RING];
#pragma unroll
  for (int q = 0; q < N::RING; ++q) ring[q] = sp[q * 64];
  sp += N::RING * 64;                      // sp = the op RING ahead of the next consumed one
  f32x16 lg{};
  for (int p = 0; p < N::PASSES; ++p) {
    f32x16 acc1[N::T1P];
#pragma unroll
    for (int u = 0; u < N::T1P; ++u) acc1[u] = f32x16{};
    for (int t = 0; t < N::T0; ++t) {
      f32x16 acc0{};
#pragma unroll
      for (int q = 0; q < N::KS0P; ++q) {
        acc0 = mfma_f32(ring[q % N::RING], xop[q], acc0);
        ring[q % N::RING] = sp[q * 64];
      }
      sp += N::KS0P * 64;
      float hv[16];
#pragma unroll
      for (int g = 0; g < 16; ++g)
        hv[g] = fmaxf(acc0[g] + bias[32 * t + (g & 3) + 8 * (g >> 2) + 4 * h], 0.0f);
#pragma unroll
      for (int g = 0; g < 16; ++g)
#pragma unroll
        for (int u = 0; u < N::T1P; ++u) {
          const int j = g * N::T1P + u;
          acc1[u] = mfma_f32(ring[j % N::RING], hv[g], acc1[u]);
          ring[j % N::RING] = sp[j * 64];
        }
      sp += 16 * N::T1P * 64;
    }
#pragma unroll
    for (int u = 0; u < N::T1P; ++u) {
      const int tile = p * N::T1P + u;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const float v = fmaxf(acc1[u][g] + bias[N::H0 + 32 * tile + (g & 3) + 8 * (g >> 2) + 4 * h], 0.0f);
        const int j = u * 16 + g;
        lg = mfma_f32(ring[j % N::RING], v, lg);
        ring[j % N::RING] = sp[j * 64];
      }
    }
    sp += 16 * N::T1P * 64;
  }
  emit_logits(lg, gb + N::H0 + N::H1, row, live, h, a);
}
