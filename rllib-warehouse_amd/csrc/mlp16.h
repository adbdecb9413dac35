// mlp16.h -- the bf16 network on v_mfma_f32_16x16x32_bf16 tiles (k_mlp16: the default for Medium and
// Large).  Part of policy_mlp.hip's anonymous namespace; needs mlp_common.h before it.

// The same network and dataflows as k_mlp (mlp32.h) on v_mfma_f32_16x16x32_bf16.  On gfx950 a
// loop of this shape holds a higher clock under load than the 32x32x16 loop at equal cycles per FLOP
// (MI355X_MICROARCH.md, 'DVFS give-back' item 7: 1.12-1.14x FLOP/s with the operands re-read from
// LDS), and its accumulator is 4 registers instead of 16.  Layouts (cdna_hip_programming.md §3):
// A lane l = row l&15, k 8(l>>4)+j; B lane l = column l&15, same k; C lane l = column l&15, rows
// 4(l>>4)+i.  A wave still computes 32 samples: two sample tiles s of 16 columns, each staged A
// fragment (16 hidden rows x 32 k, 1 KiB) feeding one MFMA per sample tile.  Hidden units come in
// groups of 32 = two 16-row tiles whose accumulators, bias + ReLU + bf16, are register for register
// the B fragment of one 32-k step of the next layer: element j of lane l is unit
// 32m + (j < 4 ? 4g + j : 16 + 4g + j - 4), g = l>>4 (kperm16, folded into the packed weights).
//  MODE 0: layer 0 group by group (all H0 units kept as B fragments, 2 x 4 VGPRs per group), then
//    layer 1 group by group with K = H0 at hand, each group's two tiles feeding one W2 k-step.
//  MODE 1 (Large): all layer-1 tiles live (2 x 4 VGPRs each); layer-0 groups streamed through them.
//  NS (2 or 4): 16-sample tiles per wave, each staged A fragment feeding NS MFMAs.  NS = 2 at 8 waves
//    (two per SIMD, 256 registers each); NS = 4 at 4 waves (one per SIMD, 512 registers): the same
//    256 samples per task, half the fragment reads per MFMA, and the bare loop of that shape holds
//    1,998 against 1,472 TFLOP/s on random data (tools/mfma16_ceiling.hip, profiles/r05_mfma16_ceiling.txt).
// Operands per unit: U0 per layer-0 group, U1 per layer-1 group (+ its W2), MODE 0.
template <int IN_, int H0_, int H1_, int WAVES_, int MODE_, int L0T_, int L1T_, int NS_ = 2>
struct Net16 : Stream<MODE_, H0_ / 32, H1_ / 32, L0T_, L1T_,
                      2 * ((IN_ + 2 + 31) / 32) + (MODE_ == 0 ? 0 : 2 * (H1_ / 32)), 2 * (H0_ / 32) + 1, H1_ / 32, H0_, H1_> {
  static constexpr int IN = IN_, INP = (IN_ + 2 + 31) / 32 * 32, OUT = 9;
  static constexpr int NS = NS_;
  static constexpr int KQ0 = INP / 32;              // layer-0 k-steps of 32
  static constexpr int KQX = (IN_ + 2 + 15) / 16;   // k-steps of 16 in wh_observe_x's operand
  static constexpr int G0 = H0_ / 32, G1 = H1_ / 32;  // groups of 32 hidden units
  static constexpr int WAVES = WAVES_, MT = 64 * WAVES_, ROWS = 16 * NS_ * WAVES_;
  static_assert(NS_ == 2 || NS_ == 4, "16-sample tiles per wave: two per 32-row operand tile");
};

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// two 16-row accumulator tiles of a group (+ bias) -> ReLU'd bf16 B fragment of the next layer
__device__ __forceinline__ bf16x8 group_frag(const f32x4& t0, const f32x4& t1) {
  const f32x8 v = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
  return relu_bf16(__builtin_convertvector(v, bf16x8));
}
__device__ __forceinline__ bf16x8 group_frag_bias(f32x4 t0, f32x4 t1, const float* bias, int base, int g) {
  const f32x4 b0 = *reinterpret_cast<const f32x4*>(bias + base + 4 * g);
  const f32x4 b1 = *reinterpret_cast<const f32x4*>(bias + base + 16 + 4 * g);
  return group_frag(t0 + b0, t1 + b1);
}

// Logits of sample tile s: output o of sample n sits in lane n + 16 (o >> 2), register o & 3.  Lanes
// 16s .. 16s + 15 gather their sample's nine and emit it (16 NS samples per wave).
template <int NS>
__device__ __forceinline__ void emit_logits16(const f32x4 (&lg)[NS], const float* b2, int64_t row0, int64_t rows,
                                              int lane, const MlpArgs& a) {
  const int n = lane & 15, part = lane >> 4;
  f32x16 z16{};
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    float v[9];
#pragma unroll
    for (int o = 0; o < 9; ++o) v[o] = __shfl(lg[s][o & 3], n + 16 * (o >> 2));
    if (part == s) {
#pragma unroll
      for (int o = 0; o < 9; ++o) z16[o] = v[o];
    }
  }
  const int64_t row = row0 + 16 * part + n;
  if (part < NS && row < rows) {
    float z[9];
#pragma unroll
    for (int o = 0; o < 9; ++o) z[o] = z16[o] + b2[o];
    emit_row(z, row, a);
  }
}

// The next chunk's LDS-DMA pieces, spread over the current chunk's operand groups (group gi of NG
// issues this wave's pieces j in [gi NPW / NG, (gi + 1) NPW / NG)) instead of all at the chunk's
// start, where each piece's issue competes with the chunk's first fragment reads (100-185 cycles a
// piece there against ~60 among MFMAs, MI355X_MICROARCH.md): medians of three rounds 307.4 -> 294.1 us
// (Medium) and 721.7 -> 715.9 us (Large) against all at the start (profiles/r05_mlpspread_ab.txt).
// Every chunk spreads but MODE 0's layer-0 chunks, which fetch at their start: all of layer 0's
// fragments are live there, and spreading spilled 46 more registers, Medium 299.8 -> 345.6 us
// (profiles/r05_tune_ab.txt; in two-operand groups still +6 %, profiles/r05_mlp3_ab.txt).
struct NextChunk {
  int op0;    // the chunk's first operand in the packed stream
  int dst;    // LDS stage, in 16-byte units from the kernel's LDS object
  int nops;   // 0: no next chunk
};
// One staged operand (1 KiB) by buffer-to-LDS DMA: the packed stream as a buffer resource, the
// operand's byte offset in an SGPR (soffset), the lane's 16 bytes by the one lane-offset VGPR every
// piece shares -- no 64-bit address per piece (with global_load_lds each piece's address pair was
// live across the operand stream and spread-out pieces spilled, profiles/r05_tune_ab.txt).
__device__ __forceinline__ void dma_piece(__amdgpu_buffer_rsrc_t wr, u32x4* dst, int op, int lane) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (__attribute__((address_space(3))) void*)dst, 16, lane * 16,
                                           op * 1024, 0, 0);
}
// The last kSpreadTail % of a chunk's groups issue no pieces, so the last ones have landed when the
// chunk ends (its vmcnt(0) before the barrier): 25 % -2.6 % (Medium) / -1.0 % (Large) against 0,
// 50 % no better (profiles/r05_mlptail_ab.txt).
constexpr int kSpreadTail = 25;
template <class N>
__device__ __forceinline__ void stage_slice(__amdgpu_buffer_rsrc_t wr, u32x4* lds, const NextChunk& nc, int gi,
                                            int ng_all, int w, int lane) {
  constexpr int NPW = (N::SOPS + N::WAVES - 1) / N::WAVES;   // pieces per wave, at most
  const int ng = ng_all - ng_all * kSpreadTail / 100 > 0 ? ng_all - ng_all * kSpreadTail / 100 : 1;
  if (gi >= ng) return;
  const int j0 = (gi * NPW + ng - 1) / ng, j1 = ((gi + 1) * NPW + ng - 1) / ng;
  for (int j = j0; j < j1; ++j) {
    const int o = w + N::WAVES * j;   // wave-uniform: SGPR bases, one lane offset VGPR
    if (o < nc.nops) dma_piece(wr, lds + nc.dst + o * 64, nc.op0 + o, lane);
  }
}
// (the LDS destination stays an offset from the __shared__ object: a generic pointer rebuilt from
// its low 32 bits is NULL for offset 0, and its cast to the LDS address space then yields the LDS
// null value, not offset 0)
__device__ __forceinline__ NextChunk uniform_chunk(int op0, int dst, int nops) {
  return NextChunk{__builtin_amdgcn_readfirstlane(op0), __builtin_amdgcn_readfirstlane(dst),
                   __builtin_amdgcn_readfirstlane(nops)};
}

template <class N, class G = GridOne>
__global__ __launch_bounds__(N::MT) void k_mlp16(typename G::Params p) {
  const G grid(p);                      // whose workgroup this is (mlp_common.h, grid policies)
  const MlpArgs& a = grid.job(p);
  // ONE __shared__ object (see k_mlp)
  __shared__ __attribute__((aligned(16))) u32x4 lds[N::STAGES * N::SOPS * 64 + N::H1 / 4];
  float* b1s = reinterpret_cast<float*>(lds + N::STAGES * N::SOPS * 64);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, g = lane >> 4;
  const float* gb = reinterpret_cast<const float*>(static_cast<const uint8_t*>(a.packed) + N::BIAS_OFF);
  const float* b2 = gb + N::H0 + N::H1;
  const int64_t ntask = (a.rows + N::ROWS - 1) / N::ROWS;
  const int my_tasks = (int)((ntask - grid.bid() + grid.nblk() - 1) / grid.nblk());

  for (int i = tid; i < N::H1; i += N::MT) b1s[i] = gb[N::H0 + i];
  const __amdgpu_buffer_rsrc_t wr =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.packed), (short)0, (int)N::BIAS_OFF, 0x00020000);
  auto stage_of = [&](int gg) { return lds + (gg & 1) * (N::SOPS * 64); };
  auto fetch = [&](int gg) {
    if (gg < my_tasks * N::NCH) {
      const int c = gg % N::NCH, op0 = (int)N::chunk_off(c);
      u32x4* dst = stage_of(gg);
      for (int o = w; o < N::chunk_ops(c); o += N::WAVES) dma_piece(wr, dst + o * 64, op0 + o, lane);
    }
  };
  auto next_of = [&](int gg) -> NextChunk {
    if (gg >= my_tasks * N::NCH) return NextChunk{0, 0, 0};
    const int c = gg % N::NCH;
    return uniform_chunk((int)N::chunk_off(c), (gg & 1) * (N::SOPS * 64), N::chunk_ops(c));
  };
  // a chunk's first act, for chunk gg, the one after it: spread = it comes back as the NextChunk whose
  // pieces the operand groups share out (stage_slice); else it is fetched here at once
  auto begin_chunk = [&](int gg, bool spread) -> NextChunk {
    if (spread) return next_of(gg);
    fetch(gg);
    return NextChunk{0, 0, 0};
  };
  fetch(0);
  chunk_end();

  // X^T fragments xb[q][s]: lane (n, g) holds features 32q + 8g + j of sample 16s + n of the wave
  constexpr int NS = N::NS;
  bf16x8 xb[N::KQ0][NS];
  const bool xf = a.xfrag != nullptr;
  auto load_x = [&](int64_t task_i) {
    const int64_t r0 = task_i * N::ROWS + w * (16 * NS);
    if (xf) {
      // wh_observe_x's 32x32x16 fragment order: 16-byte chunk ((tile * KQX + q16) * 64 + h * 32 + r)
      // holds features 16 q16 + 8 h + j of row r of the 32-row tile; sample tile s of the wave is
      // rows 16 (s & 1) .. + 15 of the wave's 32-row tile s >> 1
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        int64_t tile = (task_i * N::WAVES + w) * (NS / 2) + (s >> 1);
        tile = tile * 32 < a.rows ? tile : 0;
        const u32x4* src = a.xfrag + tile * (N::KQX * 64);
#pragma unroll
        for (int q = 0; q < N::KQ0; ++q) {
          const int q16 = 2 * q + (g >> 1);
          xb[q][s] = q16 < N::KQX ? frag(src + q16 * 64 + (g & 1) * 32 + 16 * (s & 1) + n) : bf16x8{};
        }
      }
    } else {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int64_t row = r0 + 16 * s + n;
        const bool lv = row < a.rows;
        const float* x = a.obs + (lv ? row : 0) * N::IN;
#pragma unroll
        for (int q = 0; q < N::KQ0; ++q) {
          f32x8 v;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int k = 32 * q + 8 * g + j;
            const float xv = x[k < N::IN ? k : N::IN - 1];
            v[j] = k < N::IN ? (lv ? xv : 0.0f) : (k < N::IN + 2 ? 1.0f : 0.0f);
          }
          xb[q][s] = __builtin_convertvector(v, bf16x8);
        }
      }
    }
  };
  if (my_tasks > 0) load_x(grid.bid());

  for (int it = 0; it < my_tasks; ++it) {
    const int64_t task = grid.bid() + (int64_t)it * grid.nblk();
    const int base = it * N::NCH;
    const bool has_next = it + 1 < my_tasks;
    NextChunk nc;                                   // of the chunk in hand
    auto spread = [&](int gi, int ng) { stage_slice<N>(wr, lds, nc, gi, ng, w, lane); };
    f32x4 lg[NS];
#pragma unroll
    for (int s2 = 0; s2 < NS; ++s2) lg[s2] = f32x4{};
    if constexpr (N::MODE == 0) {
      bf16x8 hb[N::G0][NS];
#pragma unroll
      for (int c = 0; c < N::L0C; ++c) {
        const int gg = base + c;
        nc = begin_chunk(gg + 1, false);            // (layer 0's fragments are all live: see NextChunk)
        f32x4 acc[2][NS];
        stream_ops<N::L0OPS>(stage_of(gg), lane, [&](int i, bf16x8 af) {
          const int m = i / N::U0, k = i % N::U0, rt = k / N::KQ0, q = k % N::KQ0;
#pragma unroll
          for (int s2 = 0; s2 < NS; ++s2) acc[rt][s2] = mfma16(af, xb[q][s2], q == 0 ? f32x4{} : acc[rt][s2]);
          if (k == N::U0 - 1) {
#pragma unroll
            for (int s2 = 0; s2 < NS; ++s2) hb[c * N::L0T + m][s2] = group_frag(acc[0][s2], acc[1][s2]);
          }
        }, spread);
        chunk_end();
      }
      for (int d = 0; d < N::L1C; ++d) {
        const int gg = base + N::L0C + d;
        nc = begin_chunk(gg + 1, true);
        // the next task's X during the last chunk (X is dead once layer 0 is done; loading it for
        // the whole of layer 1 would keep its registers live beside all of layer 0's fragments)
        if (d == N::L1C - 1 && has_next) load_x(task + grid.nblk());
        f32x4 acc[2][NS];
        stream_ops<N::L1OPS>(stage_of(gg), lane, [&](int i, bf16x8 af) {
          const int uu = i / N::U1, k = i % N::U1;
          if (k < 2 * N::G0) {
            const int rt = k / N::G0, m = k % N::G0;
#pragma unroll
            for (int s2 = 0; s2 < NS; ++s2) acc[rt][s2] = mfma16(af, hb[m][s2], m == 0 ? f32x4{} : acc[rt][s2]);
          } else {
            const int u = d * N::L1T + uu;
#pragma unroll
            for (int s2 = 0; s2 < NS; ++s2)
              lg[s2] = mfma16(af, group_frag_bias(acc[0][s2], acc[1][s2], b1s, 32 * u, g), lg[s2]);
          }
        }, spread);
        chunk_end();
      }
    } else {
      f32x4 acc1[2 * N::G1][NS];
#pragma unroll
      for (int v = 0; v < 2 * N::G1; ++v)
#pragma unroll
        for (int s2 = 0; s2 < NS; ++s2) acc1[v][s2] = f32x4{};
      for (int c = 0; c < N::L0C; ++c) {
        const int gg = base + c;
        nc = begin_chunk(gg + 1, true);
        f32x4 acc0[2][NS];
        bf16x8 hb0[NS];
        stream_ops<N::L0OPS, 4, 1>(stage_of(gg), lane, [&](int i, bf16x8 af) {
          const int k = i % N::U0;
          if (k < 2 * N::KQ0) {
            const int rt = k / N::KQ0, q = k % N::KQ0;
#pragma unroll
            for (int s2 = 0; s2 < NS; ++s2) acc0[rt][s2] = mfma16(af, xb[q][s2], q == 0 ? f32x4{} : acc0[rt][s2]);
            if (k == 2 * N::KQ0 - 1) {
#pragma unroll
              for (int s2 = 0; s2 < NS; ++s2) hb0[s2] = group_frag(acc0[0][s2], acc0[1][s2]);
            }
          } else {
            const int v = k - 2 * N::KQ0;
#pragma unroll
            for (int s2 = 0; s2 < NS; ++s2) acc1[v][s2] = mfma16(af, hb0[s2], acc1[v][s2]);
          }
        }, spread);
        chunk_end();
      }
      {
        const int gg = base + N::L0C;
        nc = begin_chunk(gg + 1, true);
        if (has_next) load_x(task + grid.nblk());
        stream_ops<N::L1OPS, 4, 1>(stage_of(gg), lane, [&](int u, bf16x8 af) {
#pragma unroll
          for (int s2 = 0; s2 < NS; ++s2)
            lg[s2] = mfma16(af, group_frag_bias(acc1[2 * u][s2], acc1[2 * u + 1][s2], b1s, 32 * u, g), lg[s2]);
        }, spread);
        chunk_end();
      }
    }
    emit_logits16<NS>(lg, b2, task * N::ROWS + w * (16 * NS), a.rows, lane, a);
  }
}
