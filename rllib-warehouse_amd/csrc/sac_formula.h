// sac_formula.h -- the scalar arithmetic of wh_sac_td (include/warehouse_amd.h, SAC TD TARGETS),
// written once for the device kernel (sac.h) and the host engine (host_engine.cpp), like geometry.h.
// Plain C++17 that is also device code.  RLlib's discrete SAC (sac_tf_policy, discrete branch), all
// in f32, every sum over the nine actions in ascending order.  Contraction into fused multiply-adds
// is switched off so that both engines round the same operations (they still differ by their
// expf / logf).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define WH_SAC_HD __host__ __device__
#else
#define WH_SAC_HD
#endif

namespace wh_sac {

constexpr int OUT = 9;   // actions = logits per row

// v = sum_o p[o] (min(q1t[o], q2t[o]) - alpha logp[o]), logp = log_softmax(pi); q2t NULL: q1t alone
WH_SAC_HD inline float soft_value(const float* pi, const float* q1t, const float* q2t, float alpha) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float zmax = pi[0];
  for (int o = 1; o < OUT; ++o) zmax = pi[o] > zmax ? pi[o] : zmax;
  float s = 0.0f;
  for (int o = 0; o < OUT; ++o) s += expf(pi[o] - zmax);
  const float lse = zmax + logf(s);
  float v = 0.0f;
  for (int o = 0; o < OUT; ++o) {
    const float logp = pi[o] - lse;
    const float p = expf(logp);
    const float q = (q2t && q2t[o] < q1t[o]) ? q2t[o] : q1t[o];
    const float soft = q - alpha * logp;
    v += p * soft;
  }
  return v;
}

// y = r + discount (masked ? 0 : v)
WH_SAC_HD inline float target(float reward, float discount, bool masked, float v) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float boot = discount * (masked ? 0.0f : v);
  return reward + boot;
}

// the ring's rule for stray actions (wh_replay_put): outside 0..8 = 4, stay
WH_SAC_HD inline int taken_action(int32_t a) { return (a >= 0 && a < OUT) ? a : 4; }

// the TD error of one row; q2a is read only when `twin`
WH_SAC_HD inline float td_row(float q1a, float q2a, bool twin, float y) {
  return twin ? 0.5f * (fabsf(q1a - y) + fabsf(q2a - y)) : fabsf(q1a - y);
}

// live agent rows of a sample: n NULL = NA; n[m] <= 0 (-1: an invalid index) = none; never more than NA
WH_SAC_HD inline int live_rows(const int32_t* n, int64_t m, int NA) {
  if (!n) return NA;
  const int32_t v = n[m];
  return v < 0 ? 0 : (v > NA ? NA : v);
}

// td[m] from the sum of its live rows' errors
WH_SAC_HD inline float td_mean(float sum, int live) { return live > 0 ? sum / (float)live : 0.0f; }

// ---- wh_sac_loss (include/warehouse_amd.h, SAC LOSSES)
// what a live row adds to the four sums, and the TD errors its two critic gradients are made of
struct LossRow {
  float c1, c2, f, t;   // c2 = 0 without a twin
  float e1, e2;         // qk[r,a] - y; e2 = 0 without a twin
};

// One live row: pi / q1 / q2 its nine logits (q2 is read only when `twin`), `a` the taken action 0..8,
// w the importance weight.  dpi[9] receives (scale p[j]) (g[j] - f).  lse, logp and p as in soft_value.
WH_SAC_HD inline LossRow loss_row(const float* pi, const float* q1, const float* q2, bool twin, float y, int a, float w,
                                  float alpha, float target_entropy, float scale, float* dpi) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float zmax = pi[0];
  for (int o = 1; o < OUT; ++o) zmax = pi[o] > zmax ? pi[o] : zmax;
  float s = 0.0f;
  for (int o = 0; o < OUT; ++o) s += expf(pi[o] - zmax);
  const float lse = zmax + logf(s);
  float p[OUT], g[OUT];
  LossRow r{};
  float q1a = 0.0f, q2a = 0.0f;   // qk[a], by comparison: no indexing by a value known only at run time
  for (int o = 0; o < OUT; ++o) {
    const float logp = pi[o] - lse;
    p[o] = expf(logp);
    const float qm = (twin && q2[o] < q1[o]) ? q2[o] : q1[o];
    g[o] = alpha * logp - qm;
    r.f += p[o] * g[o];
    r.t += p[o] * (logp + target_entropy);
    if (o == a) {
      q1a = q1[o];
      q2a = twin ? q2[o] : 0.0f;
    }
  }
  for (int j = 0; j < OUT; ++j) dpi[j] = (scale * p[j]) * (g[j] - r.f);
  r.e1 = q1a - y;
  r.c1 = ((0.5f * w) * r.e1) * r.e1;
  if (twin) {
    r.e2 = q2a - y;
    r.c2 = ((0.5f * w) * r.e2) * r.e2;
  }
  return r;
}

// dqk[r, a] of a live row
WH_SAC_HD inline float loss_dq(float scale, float w, float e) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return (scale * w) * e;
}

// stats[0..5] from the sums over the live rows: sum c1, sum c2, sum f, sum t, the live row count
WH_SAC_HD inline void loss_stats(const float* sums, float scale, float log_alpha, float* stats) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float T = scale * sums[3];
  stats[0] = scale * sums[0];
  stats[1] = scale * sums[1];
  stats[2] = scale * sums[2];
  stats[3] = (-log_alpha) * T;
  stats[4] = -T;
  stats[5] = sums[4];
}

// ---- wh_adam_step (include/warehouse_amd.h, ADAM): one element; sqrtf and / are correctly rounded
// (H: wh_adam_hyper)
template <class H>
WH_SAC_HD inline void adam_element(const H& h, float g, float& p, float& m, float& v) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float m1 = h.beta1 * m + h.omb1 * g;
  const float v1 = h.beta2 * v + (h.omb2 * g) * g;
  const float denom = sqrtf(v1) / h.sqrt_bc2 + h.eps;
  p = p - h.step_size * (m1 / denom);
  m = m1;
  v = v1;
}

// ---- wh_adam_step_clock: the tick (C: wh_adam_clock).  All in double -- IEEE multiply, subtract,
// divide and sqrt, correctly rounded on both engines -- and each field of h rounded to f32 once.
// 1 - beta^t * beta is a natural fused multiply-add, which would round once where the header rounds
// twice: contraction is off by the pragma under clang (the device) and by the attribute under g++ (the
// host engine), so the engines' equality does not rest on the host's -march having no FMA.
#if defined(__GNUC__) && !defined(__clang__)
#define WH_SAC_NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#else
#define WH_SAC_NO_CONTRACT
#endif
template <class C>
WH_SAC_HD WH_SAC_NO_CONTRACT inline void adam_tick(C& c, double lr, double beta1, double beta2, double eps) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double b1t = c.beta1_t * beta1, b2t = c.beta2_t * beta2;
  c.t = c.t + 1;
  c.beta1_t = b1t;
  c.beta2_t = b2t;
  c.h.beta1 = (float)beta1;
  c.h.omb1 = (float)(1.0 - beta1);
  c.h.beta2 = (float)beta2;
  c.h.omb2 = (float)(1.0 - beta2);
  c.h.eps = (float)eps;
  c.h.step_size = (float)(lr / (1.0 - b1t));
  c.h.sqrt_bc2 = (float)sqrt(1.0 - b2t);
}

}  // namespace wh_sac
