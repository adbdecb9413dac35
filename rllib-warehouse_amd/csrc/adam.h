// adam.h -- k_adam: one Adam step over up to WH_ADAM_MAX_SEGS tensors in one launch
// (include/warehouse_amd.h, ADAM).  Included by warehouse_amd.hip inside its namespace; the arithmetic
// of an element is sac_formula.h's adam_element, shared with the host engine.
//
// The tensors form one flat space of 16-byte pieces, four elements each.  In that index space (and
// only there) every segment is padded to a whole number of workgroup chunks of BT * ADAM_PPL pieces,
// so no piece and no workgroup straddles two tensors: a workgroup finds its segment by a uniform scan
// of the at most 24 first-workgroup numbers, which travel with the segment table in the kernel
// argument.  A segment whose four pointers are all 16-byte aligned moves whole pieces (its last,
// partial piece element by element); any other segment moves 4 bytes per access -- a choice that is
// uniform per workgroup.  28 bytes per element (p, m, v read and written, g read) and a dozen flops:
// bandwidth-bound by construction.
//
// Two instances of one body: k_adam takes the table of the step by value; k_adam_clock
// (wh_adam_step_clock) reads it from the wh_adam_clock that k_adam_tick, one lane launched just before
// it on the same stream, has advanced.  Stream order is the only ordering between the two.

constexpr int ADAM_PPL = 2;                       // pieces per lane
constexpr int ADAM_CHUNK = BT * ADAM_PPL * 4;     // elements a workgroup owns

struct AdamParams {
  wh_adam_seg seg[WH_ADAM_MAX_SEGS];
  uint32_t start[WH_ADAM_MAX_SEGS + 1];           // first workgroup of segment k; [nseg] = the grid
  wh_adam_hyper h;
  int32_t nseg;
};

template <bool CLOCK>
__device__ __forceinline__ void adam_body(const AdamParams& P, const wh_adam_clock* clock) {
  const uint32_t b = blockIdx.x;
  const int tid = threadIdx.x;
  int s = 0;                                      // the last segment that starts at or before b: an
  for (int k = 1; k < P.nseg; ++k) s += b >= P.start[k] ? 1 : 0;   // empty one shares its successor's start
  float* __restrict__ p = P.seg[s].p;
  float* __restrict__ m = P.seg[s].m;
  float* __restrict__ v = P.seg[s].v;
  const float* __restrict__ g = P.seg[s].g;
  const int64_t count = P.seg[s].count;
  const int64_t base = (int64_t)(b - P.start[s]) * ADAM_CHUNK;
  const wh_adam_hyper h = CLOCK ? clock->h : P.h;
  const bool vec = ((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)g) & 15u) == 0);   // (uniform)
  if (vec) {
#pragma unroll
    for (int it = 0; it < ADAM_PPL; ++it) {
      const int64_t e0 = base + (int64_t)(it * BT + tid) * 4;
      if (e0 + 4 <= count) {
        f32x4 pv = *reinterpret_cast<const f32x4*>(p + e0), mv = *reinterpret_cast<const f32x4*>(m + e0);
        f32x4 vv = *reinterpret_cast<const f32x4*>(v + e0);
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + e0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float pe = pv[j], me = mv[j], ve = vv[j];
          wh_sac::adam_element(h, gv[j], pe, me, ve);
          pv[j] = pe, mv[j] = me, vv[j] = ve;
        }
        *reinterpret_cast<f32x4*>(p + e0) = pv;
        *reinterpret_cast<f32x4*>(m + e0) = mv;
        *reinterpret_cast<f32x4*>(v + e0) = vv;
      } else {
        for (int j = 0; j < 4; ++j)
          if (e0 + j < count) wh_sac::adam_element(h, g[e0 + j], p[e0 + j], m[e0 + j], v[e0 + j]);
      }
    }
  } else {
#pragma unroll
    for (int it = 0; it < ADAM_PPL * 4; ++it) {
      const int64_t e = base + it * BT + tid;
      if (e < count) wh_sac::adam_element(h, g[e], p[e], m[e], v[e]);
    }
  }
}

__global__ __launch_bounds__(BT) void k_adam(AdamParams P) { adam_body<false>(P, nullptr); }

__global__ __launch_bounds__(BT) void k_adam_clock(AdamParams P, const wh_adam_clock* clock) { adam_body<true>(P, clock); }

// The tick of wh_adam_step_clock: one lane, sac_formula.h's adam_tick (shared with the host engine),
// plain stores.
struct AdamTickParams {
  wh_adam_clock* clock;
  double lr, beta1, beta2, eps;
};

__global__ __launch_bounds__(64) void k_adam_tick(AdamTickParams P) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  wh_adam_clock c = *P.clock;
  wh_sac::adam_tick(c, P.lr, P.beta1, P.beta2, P.eps);
  *P.clock = c;
}
