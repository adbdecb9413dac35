// sac_loss.h -- k_sac_loss, k_sac_loss_finish: the SAC losses and d(loss)/d(logits) from logits
// (include/warehouse_amd.h, SAC LOSSES).  Included by warehouse_amd.hip inside its namespace, after
// sac.h, whose geometry and span constants it uses; the arithmetic of a row is sac_formula.h's, shared
// with the host engine.
//
// One lane per row (m, i); a workgroup owns floor(256 / NA) whole samples, so its share of every
// [rows, 9] array, input or output, is one contiguous span.  The three input spans are staged into LDS
// as k_sac_td stages its five (aligned 16-byte loads, predicated head and tail, every load issued
// before the first LDS write) and each lane reads its 27 values at a stride of 9 words.  The three
// output spans go back through the same LDS arrays and leave as 16-byte stores.  An output pointer's
// 16-byte phase need not be its input's, so an output span has a placement offset of its own: output
// word e of array k lands on z[k][ooff[k] + e], which can be a NEIGHBOURING lane's input word.  Hence
// the order: every lane holds its inputs in registers, the workgroup passes a barrier, and only then is
// an output word written.
//
// The five sums (c1, c2, f, t, live rows) are reduced without atomics in a fixed order: a shuffle tree
// inside each wave, then the four waves in order by lane 0, into work[group * SAC_LOSS_PARTIALS ..];
// k_sac_loss_finish (one workgroup) adds the groups' partials, lane l taking groups l, l + 256, ... in
// order, then the same tree.  A grid of one workgroup writes stats itself.

constexpr int SACL_ARRAYS = 3;                           // pi, q1, q2 in; dpi, dq1, dq2 out
constexpr int SACL_SUMS = 5;
constexpr int SACL_WAVES = BT / 64;
static_assert(wh_abi::SAC_LOSS_PARTIALS >= SACL_SUMS, "a workgroup's partial sums fit its share of work");

struct SacLossParams {
  wh_sac_loss_args a;
  int64_t M;
  int32_t na;
  int32_t spw;   // samples per workgroup, floor(BT / na)
};

struct SacLossLds {
  alignas(16) float z[SACL_ARRAYS][SAC_PITCH];
  float red[SACL_WAVES][SACL_SUMS];
};

// The workgroup's sums in lane 0 (other lanes: unspecified): wave tree, then the waves in order.
__device__ __forceinline__ void sac_loss_reduce(float (&v)[SACL_SUMS], float (*red)[SACL_SUMS], int tid) {
#pragma unroll
  for (int k = 0; k < SACL_SUMS; ++k)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_down(v[k], d);
  if ((tid & 63) == 0)
#pragma unroll
    for (int k = 0; k < SACL_SUMS; ++k) red[tid >> 6][k] = v[k];
  __syncthreads();
  if (tid == 0)
#pragma unroll
    for (int k = 0; k < SACL_SUMS; ++k) {
      float s = red[0][k];
      for (int w = 1; w < SACL_WAVES; ++w) s += red[w][k];
      v[k] = s;
    }
}

__global__ __launch_bounds__(BT) void k_sac_loss(SacLossParams p) {
  __shared__ SacLossLds lds;
  const wh_sac_loss_args& a = p.a;
  const int tid = threadIdx.x, NA = p.na;
  const int64_t m0 = (int64_t)blockIdx.x * p.spw;                  // first sample of the workgroup
  const int ns = (int)(p.M - m0 < p.spw ? p.M - m0 : p.spw);       // its samples (>= 1)
  const int rows = ns * NA, len = rows * wh_sac::OUT;              // its rows and floats per array
  const int64_t row0 = m0 * NA;

  // ---- stage the three input spans: all global loads first, then the LDS writes (as k_sac_td)
  const float* src[SACL_ARRAYS] = {a.pi, a.q1, a.q2};
  {
    f32x4 v[SACL_ARRAYS][SAC_VPT];
    float sv[SACL_ARRAYS];
    int head[SACL_ARRAYS], sidx[SACL_ARRAYS];
#pragma unroll
    for (int k = 0; k < SACL_ARRAYS; ++k) {
      if (!src[k]) continue;                                       // (uniform)
      const float* g = src[k] + row0 * wh_sac::OUT;
      const int to16 = (int)((16u - ((uintptr_t)g & 15u)) & 15u) >> 2;   // floats up to the next 16-byte boundary
      head[k] = to16 < len ? to16 : len;
      const int nvec = (len - head[k]) >> 2;
      const f32x4* gv = reinterpret_cast<const f32x4*>(g + head[k]);
#pragma unroll
      for (int it = 0; it < SAC_VPT; ++it) {
        const int q = tid + it * BT;
        v[k][it] = q < nvec ? gv[q] : f32x4{};
      }
      // lanes 0-3: head element `tid`; lanes 4-7: tail element head + 4 nvec + tid - 4
      sidx[k] = tid < 4 ? (tid < head[k] ? tid : -1) : (tid < 8 && head[k] + 4 * nvec + tid - 4 < len ? head[k] + 4 * nvec + tid - 4 : -1);
      sv[k] = sidx[k] >= 0 ? g[sidx[k]] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < SACL_ARRAYS; ++k) {
      if (!src[k]) continue;
      const int off = (4 - head[k]) & 3;                           // span element e sits at z[k][off + e]
      const int nvec = (len - head[k]) >> 2;
      f32x4* lv = reinterpret_cast<f32x4*>(&lds.z[k][off + head[k]]);
#pragma unroll
      for (int it = 0; it < SAC_VPT; ++it) {
        const int q = tid + it * BT;
        if (q < nvec) lv[q] = v[k][it];
      }
      if (sidx[k] >= 0) lds.z[k][off + sidx[k]] = sv[k];
    }
  }
  __syncthreads();

  // ---- one row per lane: its 27 inputs into registers
  const int s = tid / NA, i = tid - s * NA;
  const bool in = tid < rows;
  const int64_t m = m0 + s, row = row0 + tid;
  const int nn = in ? wh_sac::live_rows(a.n, m, NA) : 0;
  const bool live = in && i < nn;
  const bool twin = a.q2 != nullptr;
  const int e = tid * wh_sac::OUT;
  float x[SACL_ARRAYS][wh_sac::OUT];
#pragma unroll
  for (int k = 0; k < SACL_ARRAYS; ++k) {
    int off = 0;
    if (src[k]) {
      const float* g = src[k] + row0 * wh_sac::OUT;
      const int to16 = (int)((16u - ((uintptr_t)g & 15u)) & 15u) >> 2;
      off = (4 - (to16 < len ? to16 : len)) & 3;
    }
#pragma unroll
    for (int o = 0; o < wh_sac::OUT; ++o) x[k][o] = (live && src[k]) ? lds.z[k][off + e + o] : 0.0f;
  }
  __syncthreads();   // no output word is written before every lane holds its inputs (see the top)

  // ---- the row's arithmetic; its three gradient rows into LDS at the outputs' own offsets
  float* dst[SACL_ARRAYS] = {a.dpi, a.dq1, a.dq2};
  int ohead[SACL_ARRAYS], ooff[SACL_ARRAYS];
#pragma unroll
  for (int k = 0; k < SACL_ARRAYS; ++k) {
    ohead[k] = ooff[k] = 0;
    if (!dst[k]) continue;
    const float* g = dst[k] + row0 * wh_sac::OUT;
    const int to16 = (int)((16u - ((uintptr_t)g & 15u)) & 15u) >> 2;
    ohead[k] = to16 < len ? to16 : len;
    ooff[k] = (4 - ohead[k]) & 3;
  }
  float sum[SACL_SUMS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float dpi[wh_sac::OUT];
  float d1 = 0.0f, d2 = 0.0f;
  int act = -1;
#pragma unroll
  for (int o = 0; o < wh_sac::OUT; ++o) dpi[o] = 0.0f;
  if (live) {
    const float alpha = expf(a.log_alpha[0]);
    const float w = a.weights ? a.weights[m] : 1.0f;
    act = wh_sac::taken_action(a.actions[row]);
    const wh_sac::LossRow r = wh_sac::loss_row(x[0], x[1], x[2], twin, a.y[row], act, w, alpha,
                                               a.target_entropy, a.scale, dpi);
    d1 = wh_sac::loss_dq(a.scale, w, r.e1);
    d2 = twin ? wh_sac::loss_dq(a.scale, w, r.e2) : 0.0f;
    sum[0] = r.c1;
    sum[1] = r.c2;
    sum[2] = r.f;
    sum[3] = r.t;
    sum[4] = 1.0f;
  }
  if (in) {   // dead rows: zeros
#pragma unroll
    for (int o = 0; o < wh_sac::OUT; ++o) {
      if (a.dpi) lds.z[0][ooff[0] + e + o] = dpi[o];
      if (a.dq1) lds.z[1][ooff[1] + e + o] = o == act ? d1 : 0.0f;
      if (a.dq2) lds.z[2][ooff[2] + e + o] = o == act ? d2 : 0.0f;
    }
  }
  __syncthreads();

  // ---- the three output spans: 16-byte stores from LDS, predicated head and tail
#pragma unroll
  for (int k = 0; k < SACL_ARRAYS; ++k) {
    if (!dst[k]) continue;                                         // (uniform)
    float* g = dst[k] + row0 * wh_sac::OUT;
    const int nvec = (len - ohead[k]) >> 2;
    const f32x4* lv = reinterpret_cast<const f32x4*>(&lds.z[k][ooff[k] + ohead[k]]);
    f32x4* gv = reinterpret_cast<f32x4*>(g + ohead[k]);
#pragma unroll
    for (int it = 0; it < SAC_VPT; ++it) {
      const int q = tid + it * BT;
      if (q < nvec) gv[q] = lv[q];
    }
    const int sidx = tid < 4 ? (tid < ohead[k] ? tid : -1) : (tid < 8 && ohead[k] + 4 * nvec + tid - 4 < len ? ohead[k] + 4 * nvec + tid - 4 : -1);
    if (sidx >= 0) g[sidx] = lds.z[k][ooff[k] + sidx];
  }

  // ---- the sums
  sac_loss_reduce(sum, lds.red, tid);
  if (tid == 0) {
    if (gridDim.x == 1) {
      wh_sac::loss_stats(sum, a.scale, a.log_alpha[0], a.stats);
    } else {
      float* w = reinterpret_cast<float*>(a.work) + (int64_t)blockIdx.x * wh_abi::SAC_LOSS_PARTIALS;
#pragma unroll
      for (int k = 0; k < SACL_SUMS; ++k) w[k] = sum[k];
    }
  }
}

struct SacLossFinishParams {
  const float* work;
  int64_t groups;
  const float* log_alpha;
  float scale;
  float* stats;
};

__global__ __launch_bounds__(BT) void k_sac_loss_finish(SacLossFinishParams p) {
  __shared__ float red[SACL_WAVES][SACL_SUMS];
  const int tid = threadIdx.x;
  float sum[SACL_SUMS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int64_t g = tid; g < p.groups; g += BT)
#pragma unroll
    for (int k = 0; k < SACL_SUMS; ++k) sum[k] += p.work[g * wh_abi::SAC_LOSS_PARTIALS + k];
  sac_loss_reduce(sum, red, tid);
  if (tid == 0) wh_sac::loss_stats(sum, p.scale, p.log_alpha[0], p.stats);
}
