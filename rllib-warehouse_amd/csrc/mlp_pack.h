// mlp_pack.h -- the packed weight blob of the policy network, written once for the host
// (wh_mlp_pack) and the device (wh_mlp_pack_device).  Part of policy_mlp.hip's anonymous namespace;
// needs mlp32.h, mlp16.h and mlp_f32.h (Net / Net16 / NetF), <mutex>, <utility>, <vector> and hip_rc
// before it.
//
// A blob is a stream of MFMA A operands in the order the forward kernel consumes them, then the f32
// biases.  What differs between the three blob formats is which weight lands in element j of lane l
// of an operand (a Map below: the k permutations, the b0 hi/lo columns, the zero padding) and in
// which order the operands come (the Map's walk).  Both are written here once:
//  * walk(visitor) names every operand of the stream as a PackOp {kind, a, b, c};
//  * elem(src, op, l, j) is the f32 value of one element of a named operand (host and device code);
//  * the host packer visits the walk and stores every element;
//  * the device packer visits the same walk once per shape into a table of PackOps, and its kernel
//    (k_mlp_pack) expands table[operand] with the same elem(): one lane, one 16-byte piece.
// The rounding (to_bf16) is the same integer code on both sides, so the two blobs are byte-identical.

struct PackSrc {   // f32 weights in torch nn.Linear layout, host or device memory
  const float *w0, *b0, *w1, *b1, *w2, *b2;
};

enum : uint16_t { PK_ZERO = 0, PK_W0 = 1, PK_W1 = 2, PK_W2 = 3 };
struct PackOp {    // one operand of the stream: which matrix, and which tile / k-step of it
  uint16_t kind, a, b, c;
};

__host__ __device__ inline uint16_t to_bf16(float f) {   // round to nearest even (NaN not expected in weights)
  uint32_t u = __builtin_bit_cast(uint32_t, f);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

__host__ __device__ inline float from_bf16(uint16_t b) { return __builtin_bit_cast(float, (uint32_t)b << 16); }

// W0 [H0][IN] with layer 0's bias in the two spare k columns: b0 = hi + lo, both bf16
template <class N>
__host__ __device__ inline float w0_elem(const PackSrc& p, int o, int k) {
  const float bh = from_bf16(to_bf16(p.b0[o]));
  return k < N::IN ? p.w0[(int64_t)o * N::IN + k] : k == N::IN ? bh : k == N::IN + 1 ? p.b0[o] - bh : 0.0f;
}

// the f32 tail after BIAS_OFF: b0 [H0], b1 [H1], b2 padded to 32 with zeros
template <class N>
__host__ __device__ inline float bias_elem(const PackSrc& p, int i) {
  if (i < N::H0) return p.b0[i];
  if (i < N::H0 + N::H1) return p.b1[i - N::H0];
  return i - N::H0 - N::H1 < N::OUT ? p.b2[i - N::H0 - N::H1] : 0.0f;
}

// Net blob (k_mlp): operand = 64 lanes x 8 bf16, lane l = row l&31, k 8(l>>5)+j of a 16-wide k-step.
template <class N>
struct Map32 {
  static constexpr bool BF16 = true;
  static constexpr int64_t OPS = N::STREAM_OPS;
  // k order of an accumulator-as-operand fragment (layers 1, 2)
  __host__ __device__ static int kperm(int i, int s, int l, int j) {
    return 32 * i + 16 * s + 8 * (j >> 2) + 4 * (l >> 5) + (j & 3);
  }
  __host__ __device__ static float elem(const PackSrc& p, PackOp d, int l, int j) {
    switch (d.kind) {
      case PK_W0:   // row tile a, k-step b: natural k order (X^T from memory)
        return w0_elem<N>(p, 32 * d.a + (l & 31), 16 * d.b + 8 * (l >> 5) + j);
      case PK_W1:   // W1 [H1][H0]: row tile a, k-step (b, c)
        return p.w1[(int64_t)(32 * d.a + (l & 31)) * N::H0 + kperm(d.b, d.c, l, j)];
      case PK_W2:   // W2 [9][H1]: k-step (a, b), rows padded to 32
        return (l & 31) < N::OUT ? p.w2[(int64_t)(l & 31) * N::H1 + kperm(d.a, d.b, l, j)] : 0.0f;
      default:
        return 0.0f;
    }
  }
  template <class V>
  static void walk(V&& v) {
    auto op = [](uint16_t kind, int a, int b, int c) { return PackOp{kind, (uint16_t)a, (uint16_t)b, (uint16_t)c}; };
    for (int c = 0; c < N::L0C; ++c)
      for (int m = 0; m < N::L0T; ++m) {
        const int t = c * N::L0T + m;                // layer-0 row tile
        const int64_t base = N::chunk_off(c) + (int64_t)m * N::U0;
        for (int q = 0; q < N::KQ0; ++q) v(base + q, op(PK_W0, t, q, 0));
        if (N::MODE == 1)                             // this tile's k-steps of every layer-1 row tile
          for (int n = 0; n < N::T1; ++n)
            for (int s = 0; s < 2; ++s) v(base + N::KQ0 + 2 * n + s, op(PK_W1, n, t, s));
      }
    if (N::MODE == 0) {
      for (int d = 0; d < N::L1C; ++d)
        for (int nn = 0; nn < N::L1T; ++nn) {
          const int n = d * N::L1T + nn;             // layer-1 row tile
          const int64_t base = N::chunk_off(N::L0C + d) + (int64_t)nn * N::U1;
          for (int t = 0; t < N::T0; ++t)
            for (int s = 0; s < 2; ++s) v(base + 2 * t + s, op(PK_W1, n, t, s));
          for (int s = 0; s < 2; ++s) v(base + 2 * N::T0 + s, op(PK_W2, n, s, 0));
        }
    } else {
      for (int n = 0; n < N::T1; ++n)
        for (int s = 0; s < 2; ++s) v(N::chunk_off(N::L0C) + 2 * n + s, op(PK_W2, n, s, 0));
    }
  }
};

// Net16 blob (k_mlp16): operands of 16 rows x 32 k, lane l = row l&15, k 8(l>>4)+j; layer-0 k order
// natural (X^T from memory), layers 1-2 in kperm16 order (the accumulator-as-operand fragments).
template <class N>
struct Map16 {
  static constexpr bool BF16 = true;
  static constexpr int64_t OPS = N::STREAM_OPS;
  __host__ __device__ static int kperm16(int m, int l, int j) {
    const int g = l >> 4;
    return 32 * m + (j < 4 ? 4 * g + j : 16 + 4 * g + j - 4);
  }
  __host__ __device__ static float elem(const PackSrc& p, PackOp d, int l, int j) {
    switch (d.kind) {
      case PK_W0:   // row tile a, k-step b (+ b0 hi/lo columns)
        return w0_elem<N>(p, 16 * d.a + (l & 15), 32 * d.b + 8 * (l >> 4) + j);
      case PK_W1:   // W1 [H1][H0] row tile a, k-step b (layer-0 group)
        return p.w1[(int64_t)(16 * d.a + (l & 15)) * N::H0 + kperm16(d.b, l, j)];
      case PK_W2:   // W2 [9][H1], rows padded to 16, k-step a
        return (l & 15) < N::OUT ? p.w2[(int64_t)(l & 15) * N::H1 + kperm16(d.a, l, j)] : 0.0f;
      default:
        return 0.0f;
    }
  }
  template <class V>
  static void walk(V&& v) {
    auto op = [](uint16_t kind, int a, int b) { return PackOp{kind, (uint16_t)a, (uint16_t)b, 0}; };
    for (int c = 0; c < N::L0C; ++c)
      for (int mm = 0; mm < N::L0T; ++mm) {
        const int t = c * N::L0T + mm;                     // layer-0 group
        const int64_t base = N::chunk_off(c) + (int64_t)mm * N::U0;
        for (int rt = 0; rt < 2; ++rt)
          for (int q = 0; q < N::KQ0; ++q) v(base + rt * N::KQ0 + q, op(PK_W0, 2 * t + rt, q));
        if (N::MODE == 1)
          for (int u = 0; u < 2 * N::G1; ++u) v(base + 2 * N::KQ0 + u, op(PK_W1, u, t));
      }
    if (N::MODE == 0) {
      for (int d = 0; d < N::L1C; ++d)
        for (int uu = 0; uu < N::L1T; ++uu) {
          const int u = d * N::L1T + uu;                   // layer-1 group
          const int64_t base = N::chunk_off(N::L0C + d) + (int64_t)uu * N::U1;
          for (int rt = 0; rt < 2; ++rt)
            for (int m = 0; m < N::G0; ++m) v(base + rt * N::G0 + m, op(PK_W1, 2 * u + rt, m));
          v(base + 2 * N::G0, op(PK_W2, u, 0));
        }
    } else {
      for (int u = 0; u < N::G1; ++u) v(N::chunk_off(N::L0C) + u, op(PK_W2, u, 0));
    }
  }
};

// NetF blob (k_mlp_f32): operand = 64 f32, lane l = row l&31, k half l>>5; the RING operands of
// read-ahead padding after the stream are never visited and stay PK_ZERO.
template <class N>
struct MapF {
  static constexpr bool BF16 = false;
  static constexpr int64_t OPS = N::OPS + N::RING;
  __host__ __device__ static int rg(int g) { return (g & 3) + 8 * (g >> 2); }   // accumulator register g -> row (half 0)
  __host__ __device__ static float elem(const PackSrc& p, PackOp d, int l, int) {
    const int i = l & 31, h = l >> 5;
    switch (d.kind) {
      case PK_W0: {   // W0 [H0][IN]: lane (i, h) = W0[32a + i][2b + h]
        const int k = 2 * d.b + h;
        return k < N::IN ? p.w0[(int64_t)(32 * d.a + i) * N::IN + k] : 0.0f;
      }
      case PK_W1:     // W1 [H1][H0]: row tile a, k pair (r_c, r_c + 4) of layer-0 tile b
        return p.w1[(int64_t)(32 * d.a + i) * N::H0 + 32 * d.b + rg(d.c) + 4 * h];
      case PK_W2:     // W2 [9][H1], rows padded to 32 with zeros: k pair (r_b, r_b + 4) of tile a
        return i < N::OUT ? p.w2[(int64_t)i * N::H1 + 32 * d.a + rg(d.b) + 4 * h] : 0.0f;
      default:
        return 0.0f;
    }
  }
  template <class V>
  static void walk(V&& v) {
    auto mk = [](uint16_t kind, int a, int b, int c) { return PackOp{kind, (uint16_t)a, (uint16_t)b, (uint16_t)c}; };
    int64_t op = 0;
    for (int p = 0; p < N::PASSES; ++p) {
      for (int t = 0; t < N::T0; ++t) {
        for (int q = 0; q < N::KS0P; ++q, ++op) v(op, mk(PK_W0, t, q, 0));
        for (int g = 0; g < 16; ++g)
          for (int u = 0; u < N::T1P; ++u, ++op) v(op, mk(PK_W1, p * N::T1P + u, t, g));
      }
      for (int u = 0; u < N::T1P; ++u)
        for (int g = 0; g < 16; ++g, ++op) v(op, mk(PK_W2, p * N::T1P + u, g, 0));
    }
  }
};

// ---- host: visit the walk, store every element
template <class N, class MAP>
std::vector<uint8_t> pack_host(const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                               const float* b2) {
  std::vector<uint8_t> blob(N::BYTES, 0);
  const PackSrc p{w0, b0, w1, b1, w2, b2};
  MAP::walk([&](int64_t op, PackOp d) {
    if constexpr (MAP::BF16) {
      uint16_t* f = reinterpret_cast<uint16_t*>(blob.data()) + op * 512;   // the kernel reads lane l's 16 bytes
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) f[l * 8 + j] = to_bf16(MAP::elem(p, d, l, j));
    } else {
      float* f = reinterpret_cast<float*>(blob.data()) + op * 64;
      for (int l = 0; l < 64; ++l) f[l] = MAP::elem(p, d, l, 0);
    }
  });
  float* bias = reinterpret_cast<float*>(blob.data() + N::BIAS_OFF);
  for (int i = 0; i < N::H0 + N::H1 + 32; ++i) bias[i] = bias_elem<N>(p, i);
  return blob;
}

// ---- device: one lane writes one 16-byte piece of the blob (an operand lane's 8 bf16, 4 lanes'
// f32, or 4 bias words) with one vector store; consecutive lanes write consecutive pieces.  The
// reads are gathers over the f32 weights (at most 1.2 MB: they stay in L2).
struct PackArgs {
  PackSrc src;
  const PackOp* table;   // [MAP::OPS]
  u32x4* out;
};

template <class N, class MAP>
__global__ __launch_bounds__(256) void k_mlp_pack(PackArgs a) {
  constexpr int64_t STREAM_PIECES = N::BIAS_OFF / 16, PIECES = N::BYTES / 16;
  static_assert(N::BIAS_OFF % 16 == 0 && N::BYTES % 16 == 0, "the blob is whole 16-byte pieces");
  static_assert(STREAM_PIECES == MAP::OPS * (MAP::BF16 ? 64 : 16), "the table names every operand of the stream");
  const int64_t piece = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (piece >= PIECES) return;
  u32x4 out;
  if (piece < STREAM_PIECES) {
    if constexpr (MAP::BF16) {
      const PackOp d = a.table[piece >> 6];
      const int l = (int)(piece & 63);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        out[j] = (uint32_t)to_bf16(MAP::elem(a.src, d, l, 2 * j)) | ((uint32_t)to_bf16(MAP::elem(a.src, d, l, 2 * j + 1)) << 16);
    } else {
      const PackOp d = a.table[piece >> 4];
      const int l0 = 4 * (int)(piece & 15);
#pragma unroll
      for (int j = 0; j < 4; ++j) out[j] = __builtin_bit_cast(uint32_t, MAP::elem(a.src, d, l0 + j, 0));
    }
  } else {
    const int i0 = 4 * (int)(piece - STREAM_PIECES);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = __builtin_bit_cast(uint32_t, bias_elem<N>(a.src, i0 + j));
  }
  a.out[piece] = out;
}

// The operand table of a blob format on the stream's device, built from the walk and uploaded on
// the first call for that shape and device (hipMalloc + a synchronous copy: not inside a stream
// capture); later calls find it here and touch nothing.
template <class MAP>
int pack_table(hipStream_t stream, const PackOp** out) {
  static std::mutex mu;
  static std::vector<std::pair<int, PackOp*>> seen;
  int dev = 0;
  hipError_t he = stream ? hipStreamGetDevice(stream, &dev) : hipGetDevice(&dev);
  if (he != hipSuccess) return hip_rc(he);
  std::lock_guard<std::mutex> lk(mu);
  for (const auto& s : seen)
    if (s.first == dev) {
      *out = s.second;
      return WH_OK;
    }
  std::vector<PackOp> tab((size_t)MAP::OPS, PackOp{PK_ZERO, 0, 0, 0});
  MAP::walk([&](int64_t op, PackOp d) { tab[(size_t)op] = d; });
  int cur = 0;
  he = hipGetDevice(&cur);
  if (he != hipSuccess) return hip_rc(he);
  if (cur != dev && (he = hipSetDevice(dev)) != hipSuccess) return hip_rc(he);
  PackOp* d = nullptr;
  he = hipMalloc(&d, tab.size() * sizeof(PackOp));
  if (he == hipSuccess) he = hipMemcpy(d, tab.data(), tab.size() * sizeof(PackOp), hipMemcpyHostToDevice);
  if (cur != dev) (void)hipSetDevice(cur);
  if (he != hipSuccess) return hip_rc(he);
  seen.emplace_back(dev, d);
  *out = d;
  return WH_OK;
}

template <class N, class MAP>
int pack_device(const PackSrc& src, void* packed, hipStream_t stream) {
  const PackOp* table = nullptr;
  const int rc = pack_table<MAP>(stream, &table);
  if (rc) return rc;
  const PackArgs a{src, table, static_cast<u32x4*>(packed)};
  constexpr int64_t PIECES = N::BYTES / 16;
  hipLaunchKernelGGL((k_mlp_pack<N, MAP>), dim3((unsigned)((PIECES + 255) / 256)), dim3(256), 0, stream, a);
  return hip_rc(hipGetLastError());
}
