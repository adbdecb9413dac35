// mlp32.h -- the bf16 network on v_mfma_f32_32x32x16_bf16 tiles (k_mlp: the default for Small, and
// the WH_MLP_LEGACY route for Medium and Large).  Part of policy_mlp.hip's anonymous namespace;
// needs mlp_common.h before it.

// One launch shape per network; every layer runs exactly once per sample.  A wave computes 32
// samples (the MFMA tile's columns); WAVES waves per workgroup share every staged weight operand,
// which streams through two LDS stages in consumption order.  Two dataflows, by which layer's
// activations fit the registers:
//  MODE 0 (H0 <= 512): layer 0 first, all H0 hidden units kept as bf16 B-operand fragments (T0 x 8
//    VGPRs); then layer 1 row tile by row tile with K = H0 at hand, each tile's bias + ReLU
//    feeding its two layer-2 MFMAs at once.  Stream: L0C chunks of L0T layer-0 tiles, then L1C
//    chunks of L1T layer-1 row tiles, each followed by its two W2 operands.
//  MODE 1 (H1 <= 256, Large): all T1 layer-1 accumulators live (T1 x 16 registers); layer-0 tiles
//    are produced one at a time and consumed at once by every layer-1 tile.  Stream: chunks of L0T
//    units {W0 tile t [KQ0], W1 k-steps of t for every row tile [T1][2]}, then W2 [T1][2].
// Operands (1 KiB MFMA A fragments) per unit: U0 per layer-0 tile, U1 per layer-1 row tile (+ its W2).
template <int IN_, int H0_, int H1_, int WAVES_, int MODE_, int L0T_, int L1T_, bool XPF_ = false>
struct Net : Stream<MODE_, H0_ / 32, H1_ / 32, L0T_, L1T_,
                    (IN_ + 2 + 15) / 16 + (MODE_ == 0 ? 0 : 2 * (H1_ / 32)), 2 * (H0_ / 32) + 2, 2 * (H1_ / 32), H0_, H1_> {
  // inputs padded to whole k-steps, with two spare columns IN, IN+1 = 1.0 carrying b0 as a
  // bf16 hi + lo pair, so layer 0's bias is added inside the MFMA at ~f32 precision
  static constexpr int IN = IN_, INP = (IN_ + 2 + 15) / 16 * 16, OUT = 9;
  static constexpr int KQ0 = INP / 16;        // layer-0 k-steps
  static constexpr int T0 = H0_ / 32, T1 = H1_ / 32;
  static constexpr int WAVES = WAVES_, MT = 64 * WAVES_, ROWS = 32 * WAVES_;   // samples per task
  // MODE 0: load the next task's X during layer 1 (registers permitting: measured a gain where
  // T0 x 8 leaves room -- Small -- and a loss at Medium, whose 256 registers then spill)
  static constexpr bool XPF = XPF_ && MODE_ == 0;
};

__device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// Layer-0 tile (bias already inside the MFMA) -> the two bf16 B-operand fragments (k-steps s = 0, 1)
// of the next layer.
__device__ __forceinline__ void relu_to_frags_nb(f32x16 t, bf16x8& f0, bf16x8& f1) {
  f32x8 lo, hi;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    lo[j] = t[j];
    hi[j] = t[8 + j];
  }
  f0 = relu_bf16(__builtin_convertvector(lo, bf16x8));
  f1 = relu_bf16(__builtin_convertvector(hi, bf16x8));
}

// The same after the bias of a tile whose rows start at hidden unit `base`.  Accumulator register g
// of lane half h holds row (g&3) + 8(g>>2) + 4h.
__device__ __forceinline__ void relu_to_frags(f32x16 t, const float* bias, int base, int h,
                                              bf16x8& f0, bf16x8& f1) {
#pragma unroll
  for (int G = 0; G < 4; ++G) {
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + base + 8 * G + 4 * h);
#pragma unroll
    for (int e = 0; e < 4; ++e) t[4 * G + e] += bv[e];
  }
  relu_to_frags_nb(t, f0, f1);
}

// Chunk c of the packed stream, global -> LDS stage by LDS-DMA: wave w copies every WAVES-th
// operand, one global_load_lds_dwordx4 (1 KiB, lane-linear) per operand.
template <class N>
__device__ __forceinline__ void stage_chunk(const u32x4* __restrict__ src, u32x4* dst, int nops, int w, int lane) {
  for (int o = w; o < nops; o += N::WAVES)
    __builtin_amdgcn_global_load_lds(src + o * 64 + lane, dst + o * 64, 16, 0, 0);
}

template <class N, class G = GridOne>
__global__ __launch_bounds__(N::MT) void k_mlp(typename G::Params p) {
  const G grid(p);                      // whose workgroup this is (mlp_common.h, grid policies)
  const MlpArgs& a = grid.job(p);
  // two weight stages + b1; A fragments are ds_read_b128 at operand*1 KiB + lane*16: conflict-free,
  // and each 1 KiB operand is read by all WAVES waves.
  // ONE __shared__ object: with a second one beside the LDS-DMA target, hipcc (ROCm 7.2) emits
  // vmcnt(0) before ds_reads and the staging stops overlapping (cdna_hip_programming.md §5, trap (a))
  __shared__ __attribute__((aligned(16))) u32x4 lds[N::STAGES * N::SOPS * 64 + N::H1 / 4];
  float* b1s = reinterpret_cast<float*>(lds + N::STAGES * N::SOPS * 64);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform (LDS-DMA base in m0)
  const int r = lane & 31, h = lane >> 5;
  const u32x4* chunks = static_cast<const u32x4*>(a.packed);
  const float* gb = reinterpret_cast<const float*>(static_cast<const uint8_t*>(a.packed) + N::BIAS_OFF);
  const float* b2 = gb + N::H0 + N::H1;
  // Persistent: one workgroup per CU walks the ROWS-sample tasks, so the weight pipeline (and b1)
  // carry over from task to task instead of restarting behind every workgroup's prologue.
  const int64_t ntask = (a.rows + N::ROWS - 1) / N::ROWS;
  const int my_tasks = (int)((ntask - grid.bid() + grid.nblk() - 1) / grid.nblk());

  for (int i = tid; i < N::H1; i += N::MT) b1s[i] = gb[N::H0 + i];
  auto stage_of = [&](int gg) { return lds + (gg & 1) * (N::SOPS * 64); };
  // running chunk counter gg = task_iter * NCH + c; chunk gg is stream chunk gg % NCH
  auto fetch = [&](int gg) {
    if (gg < my_tasks * N::NCH) {
      const int c = gg % N::NCH;
      stage_chunk<N>(chunks + N::chunk_off(c) * 64, stage_of(gg), N::chunk_ops(c), w, lane);
    }
  };
  fetch(0);
  chunk_end();                                    // chunk 0 landed

  // X^T fragments: lane (r,h) holds obs[row][16q+8h+j] (bias columns IN, IN+1 = 1.0)
  // (raw values of k-steps [q0, q1) at xr[(q - q0) * 8 + j])
  auto load_x = [&](int64_t xrow, float* xr, int q0 = 0, int q1 = N::KQ0) {
    const float* x = a.obs + (xrow < a.rows ? xrow : 0) * N::IN;
#pragma unroll
    for (int q = q0; q < q1; ++q)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 16 * q + 8 * h + j;
        xr[(q - q0) * 8 + j] = x[k < N::IN ? k : N::IN - 1];   // clamp, then select (cvt_x)
      }
  };
  auto cvt_x = [&](const float* xr, bool lv, bf16x8 (&xb)[N::KQ0], int q0 = 0, int q1 = N::KQ0) {
#pragma unroll
    for (int q = q0; q < q1; ++q) {
      f32x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 16 * q + 8 * h + j;
        v[j] = k < N::IN ? (lv ? xr[(q - q0) * 8 + j] : 0.0f) : (k < N::IN + 2 ? 1.0f : 0.0f);
      }
      xb[q] = __builtin_convertvector(v, bf16x8);
    }
  };
  // fragment-order X (wh_observe_x): the wave's 32 rows are tile task * WAVES + w, one coalesced
  // 16-byte load per k-step (tiles past the last row read tile 0: those rows are never emitted)
  const bool xf = a.xfrag != nullptr;
  auto load_xf = [&](int64_t task_i, bf16x8 (&xb)[N::KQ0]) {
    int64_t tile = task_i * N::WAVES + w;
    tile = tile * 32 < a.rows ? tile : 0;
    const u32x4* src = a.xfrag + tile * (N::KQ0 * 64) + lane;
#pragma unroll
    for (int q = 0; q < N::KQ0; ++q) xb[q] = frag(src + q * 64);
  };
  bf16x8 xb[N::KQ0];
  if (my_tasks > 0) {
    if (xf) {
      load_xf(grid.bid(), xb);
    } else {
      const int64_t row0 = (int64_t)grid.bid() * N::ROWS + w * 32 + r;
      float xr[N::KQ0 * 8];
      load_x(row0, xr);
      cvt_x(xr, row0 < a.rows, xb);
    }
  }

  for (int it = 0; it < my_tasks; ++it) {
    const int64_t task = grid.bid() + (int64_t)it * grid.nblk();
    const int64_t row = task * N::ROWS + w * 32 + r;
    const bool live = row < a.rows;               // (a wave past the end still joins the barriers)
    const int base = it * N::NCH;
    if (!xf && !N::XPF && it > 0) {               // X of this task, loaded now
      float xr[N::KQ0 * 8];
      load_x(row, xr);
      cvt_x(xr, live, xb);
    }
    // MODE 0: the NEXT task's rows are loaded during layer-1 chunks and converted after their
    // barriers (X is dead once layer 0 is done), so no task starts behind an HBM round trip; in NS
    // parts of QP k-steps, part p during chunk PF + p, to keep the raw f32 values within the
    // register budget
    constexpr int NS = N::L1C >= 3 ? 2 : 1;      // parts, one per chunk
    constexpr int QP = (N::KQ0 + NS - 1) / NS, PF = N::L1C - 1 - NS;  // k-steps per part, first chunk
    static_assert(N::MODE == 1 || PF >= 0, "layer-1 chunks to prefetch in");
    const int64_t row_next = row + (int64_t)grid.nblk() * N::ROWS;
    const bool has_next = it + 1 < my_tasks;

    f32x16 lg{};
    if constexpr (N::MODE == 0) {
      // layer 0, once: every hidden unit of the wave's 32 samples as bf16 fragments in registers
      bf16x8 hb[N::T0][2];
#pragma unroll
      for (int c = 0; c < N::L0C; ++c) {
        const int g = base + c;
        fetch(g + 1);
        f32x16 acc{};
        stream_ops<N::L0OPS>(stage_of(g), lane, [&](int i, bf16x8 af) {
          const int m = i / N::KQ0, q = i % N::KQ0;
          acc = mfma(af, xb[q], q == 0 ? f32x16{} : acc);
          if (q == N::KQ0 - 1) relu_to_frags_nb(acc, hb[c * N::L0T + m][0], hb[c * N::L0T + m][1]);
        });
        chunk_end();                              // chunk g+1 landed, stage g is free for chunk g+2
      }
      // layer 1 row tile by row tile (K = H0 from the registers), each tile's bias + ReLU feeding
      // its two layer-2 MFMAs at once
      for (int d = 0; d < N::L1C; ++d) {
        const int g = base + N::L0C + d;
        fetch(g + 1);
        // fragment-order X: the next task's operand straight into xb during the last chunk
        if (xf && d == N::L1C - 1 && has_next) load_xf(task + grid.nblk(), xb);
        float xr[QP * 8];                         // one part at a time
        if (!xf && N::XPF && d == PF && has_next) load_x(row_next, xr, 0, QP);
        if (!xf && N::XPF && NS == 2 && d == PF + 1 && has_next) load_x(row_next, xr, QP, N::KQ0);
        f32x16 acc{};
        bf16x8 f0, f1;
        // with the X prefetch: 4-op groups one group ahead (fewer fragments in flight)
        stream_ops<N::L1OPS, 4, N::XPF ? 1 : 2>(stage_of(g), lane, [&](int i, bf16x8 af) {
          const int nn = i / N::U1, k = i % N::U1;
          if (k < 2 * N::T0) {
            // (one chain per tile: splitting it into two accumulators, even / odd k-steps, measured
            // 2-6 % slower -- the dependent MFMAs are not what binds)
            acc = mfma(af, hb[k >> 1][k & 1], k == 0 ? f32x16{} : acc);
            if (k == 2 * N::T0 - 1) relu_to_frags(acc, b1s, 32 * (d * N::L1T + nn), h, f0, f1);
          } else {
            lg = mfma(af, k == 2 * N::T0 ? f0 : f1, lg);
          }
        });
        chunk_end();
        if (!xf && N::XPF && d == PF && has_next) cvt_x(xr, row_next < a.rows, xb, 0, QP);
        if (!xf && N::XPF && NS == 2 && d == PF + 1 && has_next) cvt_x(xr, row_next < a.rows, xb, QP, N::KQ0);
      }
    } else {
      // every layer-1 accumulator live; layer-0 tiles streamed through them
      f32x16 acc1[N::T1];
#pragma unroll
      for (int n = 0; n < N::T1; ++n) acc1[n] = f32x16{};
      for (int c = 0; c < N::L0C; ++c) {
        const int g = base + c;
        fetch(g + 1);
        f32x16 acc0{};
        bf16x8 hb0, hb1;
        stream_ops<N::L0OPS>(stage_of(g), lane, [&](int i, bf16x8 af) {
          const int k = i % N::U0;
          if (k < N::KQ0) {
            acc0 = mfma(af, xb[k], k == 0 ? f32x16{} : acc0);
            if (k == N::KQ0 - 1) relu_to_frags_nb(acc0, hb0, hb1);
          } else {
            const int j = k - N::KQ0;
            acc1[j >> 1] = mfma(af, (j & 1) ? hb1 : hb0, acc1[j >> 1]);
          }
        });
        chunk_end();
      }
      {
        const int g = base + N::L0C;
        fetch(g + 1);
        if (xf && has_next) load_xf(task + grid.nblk(), xb);   // X is dead once layer 0 is done
        bf16x8 f0, f1;
        stream_ops<N::L1OPS>(stage_of(g), lane, [&](int i, bf16x8 af) {
          if ((i & 1) == 0) relu_to_frags(acc1[i >> 1], b1s, 32 * (i >> 1), h, f0, f1);
          lg = mfma(af, (i & 1) ? f1 : f0, lg);
        });
        chunk_end();
      }
    }

    emit_logits(lg, b2, row, live, h, a);
  }
}
