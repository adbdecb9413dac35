// sac.h -- k_sac_td: SAC TD targets and TD errors from logits (include/warehouse_amd.h, SAC TD
// TARGETS).  Included by warehouse_amd.hip inside its namespace, after prio.h; the arithmetic of a
// row is sac_formula.h's, shared with the host engine.
//
// One lane per row (m, i).  A workgroup owns a whole number of samples, floor(256 / NA) of them, so
// td[m] is summed inside the workgroup, in ascending row order and without atomics.  Each logit
// array is contiguous [rows, 9], so a workgroup's share of it is one contiguous span: the span is
// staged into LDS with coalesced 16-byte loads (its unaligned head and tail by predicated scalar
// loads), every load issued before the first LDS write, and each lane then reads its nine values at a
// stride of 9 words, which is conflict-free.  The span is placed in LDS at the offset that makes
// its 16-byte-aligned global pieces 16-byte aligned there too.

constexpr int SAC_ARRAYS = 5;                            // pi_next, q1t_next, q2t_next, q1, q2
constexpr int SAC_SPAN = BT * wh_sac::OUT;               // floats of one array a workgroup can own
constexpr int SAC_VPT = (SAC_SPAN / 4 + BT - 1) / BT;    // 16-byte pieces per lane and array
constexpr int SAC_PITCH = SAC_SPAN + 4;                  // + the placement offset (0..3), a multiple of 4

struct SacParams {
  wh_sac_td_args a;
  int64_t M;
  int32_t na;
  int32_t spw;   // samples per workgroup, floor(BT / na)
};

struct SacLds {
  alignas(16) float z[SAC_ARRAYS][SAC_PITCH];
  float tdr[BT];   // the per-row errors, for agent counts that do not divide 16
};

__global__ __launch_bounds__(BT) void k_sac_td(SacParams p) {
  __shared__ SacLds lds;
  const wh_sac_td_args& a = p.a;
  const int tid = threadIdx.x, NA = p.na;
  const int64_t m0 = (int64_t)blockIdx.x * p.spw;                  // first sample of the workgroup
  const int ns = (int)(p.M - m0 < p.spw ? p.M - m0 : p.spw);       // its samples (>= 1)
  const int rows = ns * NA, len = rows * wh_sac::OUT;              // its rows and floats per array
  const int64_t row0 = m0 * NA;

  // ---- stage the five spans: all global loads first, then the LDS writes
  const float* src[SAC_ARRAYS] = {a.pi_next, a.q1t_next, a.q2t_next, a.q1, a.q2};
  f32x4 v[SAC_ARRAYS][SAC_VPT];
  float sv[SAC_ARRAYS];
  int head[SAC_ARRAYS], sidx[SAC_ARRAYS];
#pragma unroll
  for (int k = 0; k < SAC_ARRAYS; ++k) {
    if (!src[k]) continue;                                         // (uniform)
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
  int off[SAC_ARRAYS];                                             // span element e sits at z[k][off[k] + e]
#pragma unroll
  for (int k = 0; k < SAC_ARRAYS; ++k) {
    off[k] = 0;
    if (!src[k]) continue;
    off[k] = (4 - head[k]) & 3;
    const int nvec = (len - head[k]) >> 2;
    f32x4* lv = reinterpret_cast<f32x4*>(&lds.z[k][off[k] + head[k]]);
#pragma unroll
    for (int it = 0; it < SAC_VPT; ++it) {
      const int q = tid + it * BT;
      if (q < nvec) lv[q] = v[k][it];
    }
    if (sidx[k] >= 0) lds.z[k][off[k] + sidx[k]] = sv[k];
  }
  __syncthreads();

  // ---- one row per lane
  const int s = tid / NA, i = tid - s * NA;
  const bool live = tid < rows;
  const int64_t m = m0 + s, row = row0 + tid;
  const int nn = live ? wh_sac::live_rows(a.n, m, NA) : 0;
  float y = 0.0f, tdr = 0.0f;
  if (live && i < nn) {
    const int e = tid * wh_sac::OUT;
    const float vsoft = wh_sac::soft_value(&lds.z[0][off[0] + e], &lds.z[1][off[1] + e],
                                           a.q2t_next ? &lds.z[2][off[2] + e] : nullptr, a.alpha);
    const bool masked = a.mask_dones != 0 && a.dones[m] != 0;
    y = wh_sac::target(a.rewards[row], a.discount, masked, vsoft);
    if (a.q1) {
      const int act = wh_sac::taken_action(a.actions[row]);
      const bool twin = a.q2 != nullptr;
      tdr = wh_sac::td_row(lds.z[3][off[3] + e + act], twin ? lds.z[4][off[4] + e + act] : 0.0f, twin, y);
    }
  }
  if (live) {
    if (a.y) a.y[row] = y;
    if (a.td_rows) a.td_rows[row] = tdr;
  }
  if (!a.td) return;                                               // (uniform)

  // ---- td[m]: the sample's NA consecutive lanes, summed in ascending order by its first lane
  float sum = 0.0f;
  if ((16 % NA) == 0) {          // a sample lies within one 16-lane row of its wave
    const int first = (tid & 63) - i;
    for (int j = 0; j < NA; ++j) sum += __shfl(tdr, first + j);
  } else {
    lds.tdr[tid] = tdr;
    __syncthreads();
    if (live && i == 0)
      for (int j = 0; j < NA; ++j) sum += lds.tdr[tid + j];
  }
  if (live && i == 0) a.td[m] = wh_sac::td_mean(sum, nn);
}

// k_sac_la_td (wh_sac_td_la): k_sac_td with alpha = expf(log_alpha[0]) read here instead of taken by
// value, as k_sac_loss forms it.  A kernel of its own beside k_sac_td, statement for statement, and not a
// shared inlined body: moving k_sac_td's statements into a function both kernels call changed the code
// the compiler emits for k_sac_td, which must stay the parent's.  The uniform load of log_alpha[0] is
// issued with the staging loads; the expf happens once per lane before the row arithmetic.  p.a.alpha is
// not read.
__global__ __launch_bounds__(BT) void k_sac_la_td(SacParams p, const float* log_alpha) {
  __shared__ SacLds lds;
  const wh_sac_td_args& a = p.a;
  const float la = log_alpha[0];
  const int tid = threadIdx.x, NA = p.na;
  const int64_t m0 = (int64_t)blockIdx.x * p.spw;                  // first sample of the workgroup
  const int ns = (int)(p.M - m0 < p.spw ? p.M - m0 : p.spw);       // its samples (>= 1)
  const int rows = ns * NA, len = rows * wh_sac::OUT;              // its rows and floats per array
  const int64_t row0 = m0 * NA;

  // ---- stage the five spans: all global loads first, then the LDS writes
  const float* src[SAC_ARRAYS] = {a.pi_next, a.q1t_next, a.q2t_next, a.q1, a.q2};
  f32x4 v[SAC_ARRAYS][SAC_VPT];
  float sv[SAC_ARRAYS];
  int head[SAC_ARRAYS], sidx[SAC_ARRAYS];
#pragma unroll
  for (int k = 0; k < SAC_ARRAYS; ++k) {
    if (!src[k]) continue;                                         // (uniform)
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
  int off[SAC_ARRAYS];                                             // span element e sits at z[k][off[k] + e]
#pragma unroll
  for (int k = 0; k < SAC_ARRAYS; ++k) {
    off[k] = 0;
    if (!src[k]) continue;
    off[k] = (4 - head[k]) & 3;
    const int nvec = (len - head[k]) >> 2;
    f32x4* lv = reinterpret_cast<f32x4*>(&lds.z[k][off[k] + head[k]]);
#pragma unroll
    for (int it = 0; it < SAC_VPT; ++it) {
      const int q = tid + it * BT;
      if (q < nvec) lv[q] = v[k][it];
    }
    if (sidx[k] >= 0) lds.z[k][off[k] + sidx[k]] = sv[k];
  }
  __syncthreads();

  // ---- one row per lane
  const int s = tid / NA, i = tid - s * NA;
  const bool live = tid < rows;
  const int64_t m = m0 + s, row = row0 + tid;
  const int nn = live ? wh_sac::live_rows(a.n, m, NA) : 0;
  float y = 0.0f, tdr = 0.0f;
  if (live && i < nn) {
    const int e = tid * wh_sac::OUT;
    const float alpha = expf(la);
    const float vsoft = wh_sac::soft_value(&lds.z[0][off[0] + e], &lds.z[1][off[1] + e],
                                           a.q2t_next ? &lds.z[2][off[2] + e] : nullptr, alpha);
    const bool masked = a.mask_dones != 0 && a.dones[m] != 0;
    y = wh_sac::target(a.rewards[row], a.discount, masked, vsoft);
    if (a.q1) {
      const int act = wh_sac::taken_action(a.actions[row]);
      const bool twin = a.q2 != nullptr;
      tdr = wh_sac::td_row(lds.z[3][off[3] + e + act], twin ? lds.z[4][off[4] + e + act] : 0.0f, twin, y);
    }
  }
  if (live) {
    if (a.y) a.y[row] = y;
    if (a.td_rows) a.td_rows[row] = tdr;
  }
  if (!a.td) return;                                               // (uniform)

  // ---- td[m]: the sample's NA consecutive lanes, summed in ascending order by its first lane
  float sum = 0.0f;
  if ((16 % NA) == 0) {          // a sample lies within one 16-lane row of its wave
    const int first = (tid & 63) - i;
    for (int j = 0; j < NA; ++j) sum += __shfl(tdr, first + j);
  } else {
    lds.tdr[tid] = tdr;
    __syncthreads();
    if (live && i == 0)
      for (int j = 0; j < NA; ++j) sum += lds.tdr[tid + j];
  }
  if (live && i == 0) a.td[m] = wh_sac::td_mean(sum, nn);
}
