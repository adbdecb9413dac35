// policy_mlp.hip -- the SAC policy network forward on observation rows (bf16 MFMA, gfx950).
//
// What it replaces: `trainer.compute_action(obs)` of scripts/rollout.py:72 for the policy
// model of scripts/experiments/warehouse-*-sac/*.yaml (policy_model: relu MLP, hidden_layer_sizes
// [256,256] Small / [512,512] Medium / [1024,256] Large, 9 action logits), evaluated for every
// agent row of a batch: explore = 0 -> argmax (compute_action(explore=False)), explore = 1 ->
// a sample of Categorical(logits) by Gumbel-max with philox noise.
//
// Design (policy kernel):
//  * Column-major activations.  Every layer is H^T = W . X^T: the 32 samples of a wave are the
//    COLUMNS of a v_mfma_f32_32x32x16_bf16 tile, hidden units are its rows.  A 32x32 f32
//    accumulator keeps its column on the lane and its rows in the 16 registers, so after bias +
//    ReLU + v_cvt_pk_bf16_f32, registers 8s..8s+7 ARE the B operand of k-step s of the next layer
//    (cdna_hip_programming.md §3, "accumulator tile as the next MFMA's operand"): activations
//    never leave registers.  The permuted k order this implies is folded into the packed weights.
//  * Every layer runs once per sample (struct Net: MODE 0 keeps all layer-0 activations, MODE 1
//    all layer-1 accumulators, whichever fits 256 registers at two waves per SIMD).
//  * Layer 0's bias rides in the MFMA (two input columns fixed at 1.0 carry b0 as bf16 hi + lo);
//    ReLU runs on the packed bf16 bits (v_pk_max_i16 with 0).
//  * Weights are packed once (wh_mlp_pack) in consumption order, one MFMA A operand = 64 lanes x
//    16 contiguous bytes, and streamed chunk by chunk into two LDS stages by LDS-DMA
//    (global_load_lds_dwordx4, lane-linear); all 8 waves read every staged operand.
//  * Persistent workgroups (one per CU) walk 256-row tasks, so the weight pipeline and the
//    biases carry over from task to task.
//
// This file is the host side: the registry of kernels and the C ABI.  The kernels are in the headers
// below, one per kernel after what they share; each header's first lines say what it needs before it.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <utility>
#include <vector>

#include "abi_args.h"
#include "mlp_grid.h"
#include "philox.h"
#include "warehouse_amd.h"

namespace {

int hip_rc(hipError_t e) { return e == hipSuccess ? WH_OK : WH_EHIP + (int)e; }

#include "mlp_common.h"   // vector types, MlpArgs, the stream geometry, stream_ops, the logit tail
#include "mlp32.h"        // Net, k_mlp: bf16 on 32x32x16 tiles
#include "mlp16.h"        // Net16, k_mlp16: bf16 on 16x16x32 tiles
#include "mlp_f32.h"      // NetF, k_mlp_f32: exact f32
#include "mlp_pack.h"     // the three blob formats, the host packer and the device packer (k_mlp_pack)
#include "mlp_train.h"    // the training forward and the backward on raw nn.Linear weights (k_train*)

struct MlpKernel {
  int in, h0, h1, precision;
  int threads, rows_per_task;
  int64_t bytes;
  void (*fwd)(MlpArgs);
  void (*fwd_multi)(MlpMultiArgs);   // the same body under GridMulti (wh_mlp_forward_multi)
  std::vector<uint8_t> (*pack)(const float*, const float*, const float*, const float*, const float*, const float*);
  int (*pack_device)(const PackSrc&, void*, hipStream_t);
};

template <int IN, int H0, int H1, int WAVES, int MODE, int L0T, int L1T, bool XPF>
MlpKernel make_mlp() {
  using N = Net<IN, H0, H1, WAVES, MODE, L0T, L1T, XPF>;
  using M = Map32<N>;
  return MlpKernel{IN, H0, H1, WH_MLP_BF16, N::MT, N::ROWS, N::BYTES, k_mlp<N>, k_mlp<N, GridMulti>, pack_host<N, M>, pack_device<N, M>};
}

template <int IN, int H0, int H1, int WAVES, int MODE, int L0T, int L1T, int NS = 2>
MlpKernel make_mlp16() {
  using N = Net16<IN, H0, H1, WAVES, MODE, L0T, L1T, NS>;
  using M = Map16<N>;
  return MlpKernel{IN, H0, H1, WH_MLP_BF16, N::MT, N::ROWS, N::BYTES, k_mlp16<N>, k_mlp16<N, GridMulti>, pack_host<N, M>, pack_device<N, M>};
}

template <int IN, int H0, int H1, int PASSES>
MlpKernel make_mlp_f32() {
  using N = NetF<IN, H0, H1, PASSES>;
  using M = MapF<N>;
  return MlpKernel{IN, H0, H1, WH_MLP_F32, 256, 128, N::BYTES, k_mlp_f32<N>, k_mlp_f32<N, GridMulti>, pack_host<N, M>, pack_device<N, M>};
}

const MlpKernel* find_mlp(const wh_mlp_desc* d) {
  // the policy_model shapes of scripts/experiments/warehouse-{small,medium,large}-sac/*.yaml:
  // bf16 on 16x16x32 tiles (k_mlp16) for Medium and Large, +4-7 % over the 32x32x16 kernel on the
  // same box; Small keeps the 32x32x16 kernel, whose next-task X prefetch fits its registers there
  // (16x16x32 without it: -3 to -8 %, profiles/r04_mlp16_ab.txt).  WH_MLP_LEGACY=1 selects the
  // 32x32x16 kernel everywhere (A/B runs; a blob is packed for the kernel of its process).
  static const bool legacy = getenv("WH_MLP_LEGACY") != nullptr;
  // (One wave per SIMD -- 4 waves, 128 samples per task, 512 registers -- ran 25-28 % slower: the
  // weight stream per sample doubles, profiles/r05_mlpw4_ab.txt; four sample tiles per wave to keep
  // 256 samples per task do not fit 512 registers at Medium.)
  static const MlpKernel reg16[] = {
      make_mlp16<82, 512, 512, 8, 0, 8, 2>(),      // Medium
      make_mlp16<145, 1024, 256, 8, 1, 2, 1>(),    // Large
  };
  if (d && d->out_dim == 9 && d->precision == WH_MLP_BF16 && !legacy)
    for (const auto& k : reg16)
      if (k.in == d->in_dim && k.h0 == d->hidden0 && k.h1 == d->hidden1) return &k;
  static const MlpKernel reg[] = {
      // (waves per workgroup, dataflow MODE, layer-0 tiles per chunk, layer-1 tiles per chunk,
      // next-task X prefetch): 8 waves = two per SIMD (256 registers each)
      make_mlp<37, 256, 256, 8, 0, 8, 4, true>(),     // Small:  obs 9*4+1,  [256, 256]
      make_mlp<82, 512, 512, 8, 0, 8, 2, false>(),    // Medium: obs 9*9+1,  [512, 512]
      make_mlp<145, 1024, 256, 8, 1, 2, 1, false>(),  // Large:  obs 9*16+1, [1024, 256]
      make_mlp_f32<37, 256, 256, 1>(),    // the same shapes in exact f32
      make_mlp_f32<82, 512, 512, 2>(),
      make_mlp_f32<145, 1024, 256, 1>(),
  };
  if (!d || d->out_dim != 9) return nullptr;
  for (const auto& k : reg)
    if (k.in == d->in_dim && k.h0 == d->hidden0 && k.h1 == d->hidden1 && k.precision == d->precision) return &k;
  return nullptr;
}

// the kernel of a desc into *k, or why there is none: no desc at all, or a shape nobody registered
int lookup_mlp(const wh_mlp_desc* d, const MlpKernel** k) {
  *k = find_mlp(d);
  return *k ? WH_OK : d ? WH_ENOTSUP : WH_EINVAL;
}

}  // namespace

extern "C" {

int wh_mlp_query(const wh_mlp_desc* d, int64_t* packed_bytes) {
  const MlpKernel* k;
  if (const int rc = lookup_mlp(d, &k)) return rc;
  if (packed_bytes) *packed_bytes = k->bytes;
  return WH_OK;
}

int wh_mlp_pack(const wh_mlp_desc* d, const float* w0, const float* b0, const float* w1,
                const float* b1, const float* w2, const float* b2, void* packed) {
  const MlpKernel* k;
  if (const int rc = lookup_mlp(d, &k)) return rc;
  if (!w0 || !b0 || !w1 || !b1 || !w2 || !b2 || !packed) return WH_EINVAL;
  std::vector<uint8_t> blob = k->pack(w0, b0, w1, b1, w2, b2);
  return hip_rc(hipMemcpy(packed, blob.data(), blob.size(), hipMemcpyHostToDevice));
}

int wh_mlp_pack_device(const wh_mlp_desc* d, const float* w0, const float* b0, const float* w1,
                       const float* b1, const float* w2, const float* b2, void* packed, void* stream) {
  const MlpKernel* k;
  if (const int rc = lookup_mlp(d, &k)) return rc;
  if (!w0 || !b0 || !w1 || !b1 || !w2 || !b2 || !packed || (uintptr_t)packed % 16 != 0) return WH_EINVAL;
  return k->pack_device(PackSrc{w0, b0, w1, b1, w2, b2}, packed, (hipStream_t)stream);
}

// The argument rules of one forward on kernel k, shared by the one-network entry points and every job
// of wh_mlp_forward_multi.  *live = 0: nothing to do (rows == 0; the other fields are not looked at).
static int check_forward(const MlpKernel* k, const void* packed, int64_t rows, const float* obs, const void* xfrag,
                         const float* logits, const int32_t* actions, bool* live) {
  *live = false;
  if (rows < 0) return WH_EINVAL;
  if (rows == 0) return WH_OK;
  if (!packed || (!obs && !xfrag) || (!logits && !actions)) return WH_EINVAL;
  if (obs && xfrag) return WH_EINVAL;
  if (xfrag && (k->precision != WH_MLP_BF16 || (uintptr_t)xfrag % 16 != 0)) return WH_ENOTSUP;
  *live = true;
  return WH_OK;
}

static MlpArgs mlp_args(const void* packed, int64_t rows, const float* obs, const void* xfrag, float* logits,
                        int32_t* actions, int32_t explore, uint64_t seed, uint32_t step) {
  return MlpArgs{packed, rows, obs, logits, actions, explore ? 1 : 0, (uint32_t)(seed & 0xFFFFFFFFu),
                 (uint32_t)(seed >> 32), step, static_cast<const u32x4*>(xfrag)};
}

// CUs of the current device (one persistent workgroup per CU), asked once; 0: the runtime would not say.
// The count of the device current at the first call stays for the process: on a host with unlike
// devices a launch on another one still computes the same results (no result depends on the grid or on
// wh_mlp_forward_multi's partition, whose cap this is) and only balances its load for the first.
static int device_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  return cus;
}

static int mlp_forward(const wh_mlp_desc* d, const void* packed, int64_t rows, const float* obs,
                       const void* xfrag, float* logits, int32_t* actions, int32_t explore, uint64_t seed,
                       uint32_t step, void* stream) {
  const MlpKernel* k;
  if (const int rc = lookup_mlp(d, &k)) return rc;
  bool live;
  if (const int rc = check_forward(k, packed, rows, obs, xfrag, logits, actions, &live)) return rc;
  if (!live) return WH_OK;
  const MlpArgs a = mlp_args(packed, rows, obs, xfrag, logits, actions, explore, seed, step);
  const int cus = device_cus();
  if (!cus) return WH_EHIP;
  if (k->precision == WH_MLP_F32) {         // 32 rows per wave, 4 waves per workgroup
    const int64_t ntask = (rows + 31) / 32;
    hipLaunchKernelGGL(k->fwd, dim3((unsigned)((ntask + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    return hip_rc(hipGetLastError());
  }
  const int64_t ntask = (rows + k->rows_per_task - 1) / k->rows_per_task;
  const unsigned grid = (unsigned)(ntask < cus ? ntask : cus);
  hipLaunchKernelGGL(k->fwd, dim3(grid), dim3(k->threads), 0, (hipStream_t)stream, a);
  return hip_rc(hipGetLastError());
}

int wh_mlp_forward(const wh_mlp_desc* d, const void* packed, int64_t rows, const float* obs,
                   float* logits, int32_t* actions, int32_t explore, uint64_t seed, uint32_t step,
                   void* stream) {
  return mlp_forward(d, packed, rows, obs, nullptr, logits, actions, explore, seed, step, stream);
}

int wh_mlp_forward_x(const wh_mlp_desc* d, const void* packed, int64_t rows, const void* xfrag,
                     float* logits, int32_t* actions, int32_t explore, uint64_t seed, uint32_t step,
                     void* stream) {
  if (!xfrag) return WH_EINVAL;
  return mlp_forward(d, packed, rows, nullptr, xfrag, logits, actions, explore, seed, step, stream);
}

static_assert(mlp_grid::MAX_JOBS == WH_MLP_MAX_JOBS, "mlp_grid.h and the header agree on the job limit");

int wh_mlp_forward_multi(const wh_mlp_desc* d, int32_t njobs, const wh_mlp_job* jobs, void* stream) {
  const MlpKernel* k;
  if (const int rc = lookup_mlp(d, &k)) return rc;
  if (njobs < 0 || njobs > WH_MLP_MAX_JOBS || (njobs > 0 && !jobs)) return WH_EINVAL;
  // every job's own rules first, for all jobs, so that a job's own defect answers before the
  // shared-pointer rule below sees any pair (the header's order)
  for (int i = 0; i < njobs; ++i) {
    bool live;
    if (const int rc = check_forward(k, jobs[i].packed, jobs[i].rows, jobs[i].obs, jobs[i].xfrag, jobs[i].logits,
                                     jobs[i].actions, &live))
      return rc;
  }
  MlpMultiArgs m{};                          // the live jobs, in order
  int64_t work[WH_MLP_MAX_JOBS];             // per live job: tasks (persistent) or rows (f32)
  int n = 0;
  for (int i = 0; i < njobs; ++i) {
    const wh_mlp_job& j = jobs[i];
    bool live;
    if (const int rc = check_forward(k, j.packed, j.rows, j.obs, j.xfrag, j.logits, j.actions, &live)) return rc;
    if (!live) continue;
    for (int o = 0; o < n; ++o)             // two jobs writing one buffer: the result would be either's
      if ((j.logits && j.logits == m.job[o].logits) || (j.actions && j.actions == m.job[o].actions)) return WH_EINVAL;
    m.job[n] = mlp_args(j.packed, j.rows, j.obs, j.xfrag, j.logits, j.actions, j.explore, j.seed, j.step);
    work[n] = k->precision == WH_MLP_F32 ? j.rows : mlp_grid::ceil_div(j.rows, k->rows_per_task);
    ++n;
  }
  if (n == 0) return WH_OK;
  m.njobs = n;
  if (k->precision == WH_MLP_F32) {
    if (!mlp_grid::per_tile(n, work, m.first)) return WH_EINVAL;   // (a grid past 2^31 - 1 blocks)
    hipLaunchKernelGGL(k->fwd_multi, dim3((unsigned)m.first[n]), dim3(256), 0, (hipStream_t)stream, m);
    return hip_rc(hipGetLastError());
  }
  const int cus = device_cus();
  if (!cus) return WH_EHIP;
  if (!mlp_grid::persistent(n, work, cus < n ? n : cus, m.first)) return WH_EINVAL;
  hipLaunchKernelGGL(k->fwd_multi, dim3((unsigned)m.first[n]), dim3(k->threads), 0, (hipStream_t)stream, m);
  return hip_rc(hipGetLastError());
}

// MLP TRAINING (csrc/mlp_train.h): the argument rules are abi_args.h's, the launches mlp_train.h's
int wh_mlp_train_query(const wh_mlp_desc* d, int64_t rows, int64_t* work_bytes) {
  if (const int rc = wh_abi::mlp_train_query_call(d, rows)) return rc;
  if (work_bytes) *work_bytes = train::work_bytes(train::Dims{d->in_dim, d->hidden0, d->hidden1}, rows);
  return WH_OK;
}

int wh_mlp_train_forward(const wh_mlp_desc* d, const wh_mlp_weights* w, int64_t rows, const float* obs,
                         float* h0, float* h1, float* logits, void* stream) {
  bool live;
  if (const int rc = wh_abi::mlp_train_forward_call(d, w, rows, obs, h0, h1, logits, &live)) return rc;
  if (!live) return WH_OK;
  return train::forward(train::Dims{d->in_dim, d->hidden0, d->hidden1}, *w, rows, obs, h0, h1, logits,
                        (hipStream_t)stream);
}

int wh_mlp_backward(const wh_mlp_desc* d, const wh_mlp_weights* w, int64_t rows, const float* obs,
                    const float* h0, const float* h1, const float* dlogits, const wh_mlp_grads* g,
                    void* work, void* stream) {
  if (const int rc = wh_abi::mlp_backward_call(d, w, rows, obs, h0, h1, dlogits, g, work)) return rc;
  return train::backward(train::Dims{d->in_dim, d->hidden0, d->hidden1}, *w, rows, obs, h0, h1, dlogits, *g, work,
                         (hipStream_t)stream);
}

int wh_mlp_train_forward_multi(const wh_mlp_desc* d, int32_t nnets, const wh_mlp_train_job* jobs, int64_t rows,
                               void* stream) {
  if (const int rc = wh_abi::mlp_train_multi_call(d, nnets, jobs, rows, false)) return rc;
  if (nnets == 0 || rows == 0) return WH_OK;
  return train::forward_multi(train::Dims{d->in_dim, d->hidden0, d->hidden1}, nnets, jobs, rows, (hipStream_t)stream);
}

int wh_mlp_backward_multi(const wh_mlp_desc* d, int32_t nnets, const wh_mlp_train_job* jobs, int64_t rows,
                          void* stream) {
  if (const int rc = wh_abi::mlp_train_multi_call(d, nnets, jobs, rows, true)) return rc;
  if (nnets == 0) return WH_OK;
  return train::backward_multi(train::Dims{d->in_dim, d->hidden0, d->hidden1}, nnets, jobs, rows, (hipStream_t)stream);
}

}  // extern "C"
