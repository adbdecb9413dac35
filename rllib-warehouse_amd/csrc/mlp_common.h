// mlp_common.h -- what the policy kernels share: vector types, the launch arguments, the packed
// stream's geometry, the staged-operand loop and the logit tail.  Part of policy_mlp.hip's anonymous
// namespace; needs <hip/hip_runtime.h>, <stdint.h>, philox.h and warehouse_amd.h before it.

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

constexpr uint32_t PUR_MLP = 5;         // philox purpose (1-4 are the simulator's, device_vocab.h)

struct MlpArgs {
  const void* packed;
  int64_t rows;
  const float* obs;
  float* logits;
  int32_t* actions;
  int32_t explore;
  uint32_t k0, k1, step;
  const u32x4* xfrag;   // non-null: X already in fragment order (wh_observe_x), obs unused
};

// Grid policies: every kernel template takes one as its second parameter, and its body asks it which
// MlpArgs the workgroup works on (job), what its block index within that job is (bid) and how many
// blocks the job has (nblk) instead of reading blockIdx.x / gridDim.x.
// GridOne, the default: the whole grid is one network's (wh_mlp_forward, wh_mlp_forward_x).
struct GridOne {
  using Params = MlpArgs;
  __device__ __forceinline__ explicit GridOne(const MlpArgs&) {}
  __device__ __forceinline__ const MlpArgs& job(const MlpArgs& p) const { return p; }
  __device__ __forceinline__ unsigned bid() const { return blockIdx.x; }
  __device__ __forceinline__ unsigned nblk() const { return gridDim.x; }
};

// GridMulti (wh_mlp_forward_multi): up to WH_MLP_MAX_JOBS jobs of one network shape side by side in
// one grid, blocks first[j] .. first[j + 1] - 1 being job j's (mlp_grid.h).  The table travels by
// value as the kernel argument.  The scan depends on blockIdx.x and kernel arguments only, so the job
// is workgroup-uniform and its fields are scalar loads from the argument segment into SGPRs; the body
// then runs as it does for one network, with a job-local block index and stride.
struct MlpMultiArgs {
  MlpArgs job[WH_MLP_MAX_JOBS];
  int32_t first[WH_MLP_MAX_JOBS + 1];
  int32_t njobs;
};
struct GridMulti {
  using Params = MlpMultiArgs;
  int j;
  unsigned b0, b1;
  __device__ __forceinline__ explicit GridMulti(const MlpMultiArgs& p) {
    int jj = 0;
#pragma unroll
    for (int i = 1; i < WH_MLP_MAX_JOBS; ++i)
      if (i < p.njobs && blockIdx.x >= (unsigned)p.first[i]) jj = i;
    j = __builtin_amdgcn_readfirstlane(jj);
    b0 = (unsigned)p.first[j];
    b1 = (unsigned)p.first[j + 1];
  }
  // (by value: the job's 64 bytes are loaded into SGPRs once, as a single launch's arguments are; a
  // reference into the table re-read fields along the body and cost k_mlp16 Medium 8 more bytes of
  // scratch per lane than its one-network kernel has)
  __device__ __forceinline__ MlpArgs job(const MlpMultiArgs& p) const { return p.job[j]; }
  __device__ __forceinline__ unsigned bid() const { return blockIdx.x - b0; }
  __device__ __forceinline__ unsigned nblk() const { return b1 - b0; }
};

// The packed weight stream of a bf16 network (Net, Net16), in 1 KiB MFMA A operands: L0C chunks of
// L0T layer-0 units (N0 units of U0 operands), then in MODE 0 L1C chunks of L1T layer-1 units (N1
// units of U1 operands), in MODE 1 one chunk of TAIL operands (W2); the f32 biases b0 [H0], b1 [H1],
// b2 [32] follow at BIAS_OFF.  A chunk is what one LDS stage holds while the next one lands.
template <int MODE_, int N0, int N1, int L0T_, int L1T_, int U0_, int U1_, int TAIL, int H0_, int H1_>
struct Stream {
  static constexpr int MODE = MODE_, L0T = L0T_, L1T = L1T_, U0 = U0_, U1 = U1_, H0 = H0_, H1 = H1_;
  static constexpr int L0C = N0 / L0T, L0OPS = L0T * U0;
  static constexpr int L1C = MODE == 0 ? N1 / L1T : 1, L1OPS = MODE == 0 ? L1T * U1 : TAIL;
  static constexpr int NCH = L0C + L1C;
  static constexpr int SOPS = L0OPS > L1OPS ? L0OPS : L1OPS;   // one LDS stage
  static constexpr int64_t STREAM_OPS = (int64_t)L0C * L0OPS + (int64_t)L1C * L1OPS;
  static constexpr int64_t BIAS_OFF = STREAM_OPS * 1024;
  static constexpr int64_t BYTES = BIAS_OFF + 4 * (H0 + H1 + 32);
  static constexpr int STAGES = 2;            // chunk g in use, chunk g+1 landing
  static constexpr int LDS_BYTES = STAGES * SOPS * 1024 + 4 * H1;
  static_assert(H0 % 32 == 0 && H1 % 32 == 0 && N0 % L0T == 0 && (MODE == 1 || N1 % L1T == 0), "tile shapes");
  static_assert(LDS_BYTES <= 160 * 1024, "two weight stages + b1 must fit the 160 KiB LDS");
  __host__ __device__ static constexpr int64_t chunk_off(int c) {
    return c < L0C ? (int64_t)c * L0OPS : (int64_t)L0C * L0OPS + (int64_t)(c - L0C) * L1OPS;
  }
  __host__ __device__ static constexpr int chunk_ops(int c) { return c < L0C ? L0OPS : L1OPS; }
};

__device__ __forceinline__ bf16x8 frag(const u32x4* p) { return __builtin_bit_cast(bf16x8, *p); }

// ReLU after the bf16 rounding, on the packed bits: a bf16 with the sign bit set is a negative
// int16, so v_pk_max_i16(x, 0) is max(x, +0) for two values per op (round(max(v,0)) ==
// max(round(v),0) since rounding keeps the sign).
__device__ __forceinline__ bf16x8 relu_bf16(bf16x8 v) {
  return __builtin_bit_cast(bf16x8, __builtin_elementwise_max(__builtin_bit_cast(s16x8, v), (s16x8){}));
}

// A chunk ends: this wave's pieces of the next chunk have landed (vmcnt(0)), and after the barrier
// so have every wave's, while the stage just read is free for the chunk after that.
__device__ __forceinline__ void chunk_end() {
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();
}

// NOPS consecutive staged operands, each fed to MFMA f(i, A fragment): fragments are read from LDS
// DEPTH groups of GS ahead of their MFMAs; the sched_barriers keep the reads ahead of the MFMAs and
// stop the compiler from hoisting a whole chunk's reads (NOPS x 4 VGPRs would spill).
struct NoPre {
  __device__ __forceinline__ void operator()(int, int) const {}
};
template <int NOPS, int GS_ = 4, int DEPTH = 2, class F, class P = NoPre>
__device__ __forceinline__ void stream_ops(const u32x4* S, int lane, F&& f, P&& pre = P{}) {
  constexpr int GS = NOPS % GS_ == 0 ? GS_ : 2, NG = NOPS / GS;
  static_assert(NOPS % GS == 0 && NG >= DEPTH, "operand groups");
  bf16x8 buf[DEPTH + 1][GS];
#pragma unroll
  for (int d = 0; d < DEPTH; ++d)
#pragma unroll
    for (int i = 0; i < GS; ++i) buf[d][i] = frag(S + (d * GS + i) * 64 + lane);
#pragma unroll
  for (int gi = 0; gi < NG; ++gi) {
    if (gi + DEPTH < NG) {
#pragma unroll
      for (int i = 0; i < GS; ++i) buf[(gi + DEPTH) % (DEPTH + 1)][i] = frag(S + ((gi + DEPTH) * GS + i) * 64 + lane);
    }
    pre(gi, NG);                                   // (k_mlp16: this group's share of the next chunk's DMA)
    __builtin_amdgcn_sched_barrier(0);             // later groups' reads issue BEFORE this group's MFMAs
#pragma unroll
    for (int i = 0; i < GS; ++i) f(gi * GS + i, buf[gi % (DEPTH + 1)][i]);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// The tail of every kernel, for one sample whose nine logits z (b2 added) its lane holds: writes the
// logits and/or the argmax (first maximum) or a Gumbel-max sample.
__device__ __forceinline__ void emit_row(const float (&z)[9], int64_t row, const MlpArgs& a) {
  constexpr int OUT = 9;
  if (a.logits) {
#pragma unroll
    for (int o = 0; o < OUT; ++o) a.logits[row * OUT + o] = z[o];
  }
  if (a.actions) {
    float best = -INFINITY;
    int arg = 0;
    if (a.explore) {
      // Gumbel-max: first maximum of z_o + g_o, g = -log(-log u).  Action o takes word o of philox
      // blocks 0-2 of counter (row lo, row hi, step, PUR_MLP << 24 | block), key (seed lo, seed hi);
      // words 9-11 are unused.  u = (f32(w >> 8) + 0.5f) * 2^-24 lies in (0, 1]: for w >> 8 = 0xFFFFFF
      // the f32 sum rounds to 2^24, u = 1, g = +inf and that action is taken (once in 2^24 draws).
      // Modelled by oracle/policy_tail.py.
      uint32_t u32[12];
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const uint4 v = philox10(make_uint4((uint32_t)row, (uint32_t)(row >> 32), a.step, (PUR_MLP << 24) | (uint32_t)b),
                                 a.k0, a.k1);
        u32[4 * b] = v.x;
        u32[4 * b + 1] = v.y;
        u32[4 * b + 2] = v.z;
        u32[4 * b + 3] = v.w;
      }
#pragma unroll
      for (int o = 0; o < OUT; ++o) {
        const float u = ((float)(u32[o] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float v = z[o] - __logf(-__logf(u));
        if (v > best) { best = v; arg = o; }
      }
    } else {
#pragma unroll
      for (int o = 0; o < OUT; ++o)
        if (z[o] > best) { best = z[o]; arg = o; }   // first maximum wins (numpy/torch argmax)
    }
    a.actions[row] = arg;
  }
}

// Logits off a 32x32 output tile (k_mlp, k_mlp_f32): logit o of sample r sits as o 0-3 in lane r
// regs 0-3, o 4-7 in lane r+32 regs 0-3, o 8 in lane r reg 4 (C/D map row = (reg&3) + 8(reg>>2) +
// 4(lane>>5)).  Adds b2, then emit_row on the lanes of half 0.
__device__ __forceinline__ void emit_logits(const f32x16& lg, const float* b2, int64_t row, bool live, int h,
                                            const MlpArgs& a) {
  float up[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) up[e] = __shfl_xor(lg[e], 32);
  if (h == 0 && live) {
    float z[9];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      z[e] = lg[e] + b2[e];
      z[4 + e] = up[e] + b2[4 + e];
    }
    z[8] = lg[4] + b2[8];
    emit_row(z, row, a);
  }
}
