// The host engine's recorded step (csrc/host_engine.cpp: wh_replay_record) under AddressSanitizer +
// UndefinedBehaviorSanitizer: every variant and agent count the suite uses, external actions one step
// at a time and device-policy launches of several steps that wrap the ring, against a twin recorded
// by the five calls (policy, put, step, put, reset) -- all buffers exactly the sizes the header
// states, so any read or write past them, any overflow UB and any leak is reported.  Built and run by
// tests/test_asan_record.py; prints "ASAN RECORD OK" on a clean run.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "warehouse_amd.h"

namespace {

int fails = 0;
#define EXPECT(c)                                                  \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                     \
    }                                                              \
  } while (0)

wh_config variant(int D, int R, std::vector<int> racks, int na) {
  wh_config c{};
  c.area_dimension = D;
  c.num_requests = R;
  c.num_racks = (int32_t)racks.size();
  for (size_t i = 0; i < racks.size(); ++i) c.racks[i] = racks[i];
  c.agent_slots = na;
  c.episode_duration = 3;   // short episodes: done flags and fresh states inside the recorded steps
  c.pickup_wait_duration = 200;
  return c;
}

struct Ring {   // a ring of exactly the header's sizes
  std::vector<uint32_t> states;
  std::vector<uint8_t> actions, dones;
  std::vector<float> rewards;
  wh_replay_ring r;
  Ring(int64_t cap, int64_t B, int NA, int W)
      : states((size_t)cap * 2 * B * W), actions((size_t)cap * B * NA), dones((size_t)cap * B),
        rewards((size_t)cap * B * NA), r{states.data(), actions.data(), rewards.data(), dones.data(), cap} {}
  bool operator==(const Ring& o) const {
    return states == o.states && actions == o.actions && dones == o.dones &&
           !memcmp(rewards.data(), o.rewards.data(), rewards.size() * sizeof(float));
  }
};

void exercise(const wh_config& cfg, int64_t B, int64_t cap, bool train, uint64_t seed) {
  wh_layout L{};
  EXPECT(wh_query(&cfg, &L) == WH_OK);
  const int NA = cfg.agent_slots, OBS = L.obs_len, W = L.words_per_env;
  std::vector<uint32_t> sa((size_t)W * B), sb((size_t)W * B);   // a: wh_replay_record, b: the five calls
  Ring ra(cap, B, NA, W), rb(cap, B, NA, W);
  std::vector<float> rew((size_t)B * NA), obs((size_t)B * NA * OBS), obs_b((size_t)B * NA * OBS);
  std::vector<uint8_t> done(B);
  std::vector<int32_t> acts((size_t)B * NA);
  std::vector<uint32_t> epr_a(B), epr_b(B);
  std::vector<uint64_t> sum_a(NA + 1), sum_b(NA + 1), cnt_a(NA + 1), cnt_b(NA + 1);
  const wh_episode_stats st_a{epr_a.data(), sum_a.data(), cnt_a.data(), nullptr, nullptr};
  const wh_episode_stats st_b{epr_b.data(), sum_b.data(), cnt_b.data(), nullptr, nullptr};
  EXPECT(wh_reset(&cfg, B, sa.data(), nullptr, nullptr, train, seed, 0, nullptr) == WH_OK);
  sb = sa;
  int64_t slot = 0, dones_seen = 0;

  auto five_calls = [&](int32_t policy, float p, float* rw_out, uint8_t* dn_out) {
    if (policy) EXPECT(wh_policy(&cfg, B, sb.data(), policy, p, acts.data(), seed, 0, nullptr) == WH_OK);
    EXPECT(wh_replay_put(&cfg, B, &rb.r, slot, 0, sb.data(), acts.data(), nullptr, nullptr, nullptr) == WH_OK);
    EXPECT(wh_vector_step(&cfg, B, sb.data(), acts.data(), nullptr, 0, nullptr, rew.data(), done.data(), nullptr, &st_b,
                          0, train, seed, 0, nullptr) == WH_OK);
    EXPECT(wh_replay_put(&cfg, B, &rb.r, slot, 1, sb.data(), nullptr, rew.data(), done.data(), nullptr) == WH_OK);
    EXPECT(wh_reset(&cfg, B, sb.data(), done.data(), nullptr, train, seed, 0, nullptr) == WH_OK);
    for (int64_t e = 0; e < B; ++e) dones_seen += done[e];
    if (rw_out) EXPECT(!memcmp(rw_out, rew.data(), rew.size() * sizeof(float)));
    if (dn_out) EXPECT(!memcmp(dn_out, done.data(), done.size()));
    slot = (slot + 1) % cap;
  };
  auto same = [&]() {
    EXPECT(sa == sb);
    EXPECT(ra == rb);
    EXPECT(epr_a == epr_b && sum_a == sum_b && cnt_a == cnt_b);
  };

  // external actions, one step per call (some outside 0 .. 8), rows of the final state
  for (int s = 0; s < cap + 2; ++s) {
    EXPECT(wh_policy(&cfg, B, sa.data(), WH_POLICY_GREEDY, 0.3f, acts.data(), seed, 0, nullptr) == WH_OK);
    acts[(size_t)(s % B) * NA] = 9 + s;
    std::vector<float> rw1((size_t)B * NA);
    std::vector<uint8_t> dn1(B);
    EXPECT(wh_replay_record(&cfg, B, sa.data(), &ra.r, slot, 1, WH_POLICY_EXTERNAL, 0.0f, acts.data(), rw1.data(),
                            dn1.data(), obs.data(), nullptr, &st_a, train, seed, 0, nullptr) == WH_OK);
    five_calls(0, 0.0f, rw1.data(), dn1.data());
    EXPECT(wh_observe(&cfg, B, sb.data(), obs_b.data(), nullptr) == WH_OK);
    EXPECT(!memcmp(obs.data(), obs_b.data(), obs.size() * sizeof(float)));
    same();
  }
  // the device policies, K steps per call from wherever the cursor is: a wrapping collect
  for (int32_t policy : {WH_POLICY_GREEDY, WH_POLICY_RANDOM})
    for (int64_t K = 1; K <= cap; ++K) {
      std::vector<float> rwk((size_t)K * B * NA);
      std::vector<uint8_t> dnk((size_t)K * B);
      EXPECT(wh_replay_record(&cfg, B, sa.data(), &ra.r, slot, (int32_t)K, policy, 0.3f, nullptr, rwk.data(), dnk.data(),
                              nullptr, nullptr, &st_a, train, seed, 0, nullptr) == WH_OK);
      for (int64_t k = 0; k < K; ++k) five_calls(policy, 0.3f, &rwk[(size_t)k * B * NA], &dnk[(size_t)k * B]);
      same();
    }
  // no live outputs at all: the ring alone
  EXPECT(wh_replay_record(&cfg, B, sa.data(), &ra.r, slot, 1, WH_POLICY_RANDOM, 0.0f, nullptr, nullptr, nullptr, nullptr,
                          nullptr, nullptr, train, seed, 0, nullptr) == WH_OK);
  EXPECT(dones_seen > 0);

  // refusals and empty calls touch nothing (NULL buffers would fault)
  const wh_replay_ring none{nullptr, nullptr, nullptr, nullptr, cap};
  EXPECT(wh_replay_record(&cfg, 0, nullptr, &none, 0, 1, WH_POLICY_GREEDY, 0.0f, nullptr, nullptr, nullptr, nullptr,
                          nullptr, nullptr, 0, 0, 0, nullptr) == WH_OK);
  EXPECT(wh_replay_record(&cfg, B, sa.data(), &none, 0, 0, WH_POLICY_GREEDY, 0.0f, nullptr, nullptr, nullptr, nullptr,
                          nullptr, nullptr, 0, 0, 0, nullptr) == WH_OK);
  EXPECT(wh_replay_record(&cfg, B, sa.data(), &none, 0, 1, WH_POLICY_GREEDY, 0.0f, nullptr, nullptr, nullptr, nullptr,
                          nullptr, nullptr, 0, 0, 0, nullptr) == WH_EINVAL);
  EXPECT(wh_replay_record(&cfg, B, sa.data(), &ra.r, cap, 1, WH_POLICY_GREEDY, 0.0f, nullptr, nullptr, nullptr, nullptr,
                          nullptr, nullptr, 0, 0, 0, nullptr) == WH_EINVAL);
  EXPECT(wh_replay_record(&cfg, B, sa.data(), &ra.r, 0, (int32_t)cap + 1, WH_POLICY_GREEDY, 0.0f, nullptr, nullptr,
                          nullptr, nullptr, nullptr, nullptr, 0, 0, 0, nullptr) == WH_EINVAL);
  EXPECT(wh_replay_record(&cfg, B, sa.data(), &ra.r, 0, 1, WH_POLICY_EXTERNAL, 0.0f, nullptr, nullptr, nullptr, nullptr,
                          nullptr, nullptr, 0, 0, 0, nullptr) == WH_EINVAL);
  alignas(16) char frag[16];
  EXPECT(wh_replay_record(&cfg, B, sa.data(), &ra.r, 0, 1, WH_POLICY_GREEDY, 0.0f, nullptr, nullptr, nullptr, nullptr,
                          frag, nullptr, 0, 0, 0, nullptr) == WH_ENOTSUP);
}

}  // namespace

int main() {
  exercise(variant(12, 4, {4, 8}, 4), 37, 5, false, 11);
  exercise(variant(16, 9, {4, 8, 12}, 8), 37, 5, false, 12);
  exercise(variant(16, 9, {4, 8, 12}, 1), 5, 3, false, 13);
  exercise(variant(16, 9, {4, 8, 12}, 3), 9, 1, false, 14);
  exercise(variant(16, 9, {4, 8, 12}, 9), 37, 4, true, 15);
  exercise(variant(20, 16, {4, 8, 12, 16}, 16), 19, 2, false, 16);
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("ASAN RECORD OK\n");
  return 0;
}
