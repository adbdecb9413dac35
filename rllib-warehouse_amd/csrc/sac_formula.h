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

}  // namespace wh_sac
