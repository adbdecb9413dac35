// The host engine's replay ring (csrc/host_engine.cpp: wh_replay_put / wh_replay_gather) under
// AddressSanitizer + UndefinedBehaviorSanitizer: every variant and agent count the suite uses, a ring
// that wraps, explicit indices with duplicates and invalid entries, device-style drawn indices, every
// output set -- all buffers exactly the sizes the header states, so any read or write past them, any
// overflow UB and any leak is reported.  Built and run by tests/test_asan_replay.py; prints
// "ASAN REPLAY OK" on a clean run.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>
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

void exercise(const wh_config& cfg, int64_t B, int64_t cap, bool train, uint64_t seed) {
  wh_layout L{};
  EXPECT(wh_query(&cfg, &L) == WH_OK);
  const int NA = cfg.agent_slots, OBS = L.obs_len, W = L.words_per_env;
  std::vector<uint32_t> state((size_t)W * B);
  std::vector<float> rew((size_t)B * NA);
  std::vector<uint8_t> done(B);
  std::vector<int32_t> acts((size_t)B * NA);
  std::vector<uint32_t> r_states((size_t)cap * 2 * B * W);
  std::vector<uint8_t> r_actions((size_t)cap * B * NA), r_dones((size_t)cap * B);
  std::vector<float> r_rewards((size_t)cap * B * NA);
  const wh_replay_ring ring{r_states.data(), r_actions.data(), r_rewards.data(), r_dones.data(), cap};
  std::mt19937_64 rng(seed);

  EXPECT(wh_reset(&cfg, B, state.data(), nullptr, nullptr, train, seed, 0, nullptr) == WH_OK);
  int64_t filled = 0, dones_seen = 0;
  for (int s = 0; s < 2 * cap + 3; ++s) {   // the ring wraps twice
    const int64_t slot = s % cap;
    EXPECT(wh_policy(&cfg, B, state.data(), WH_POLICY_GREEDY, 0.3f, acts.data(), seed, 0, nullptr) == WH_OK);
    EXPECT(wh_replay_put(&cfg, B, &ring, slot, 0, state.data(), acts.data(), nullptr, nullptr, nullptr) == WH_OK);
    EXPECT(wh_vector_step(&cfg, B, state.data(), acts.data(), nullptr, 0, nullptr, rew.data(), done.data(), nullptr,
                          nullptr, 0, train, seed, 0, nullptr) == WH_OK);
    EXPECT(wh_replay_put(&cfg, B, &ring, slot, 1, state.data(), nullptr, rew.data(), done.data(), nullptr) == WH_OK);
    for (int64_t e = 0; e < B; ++e) dones_seen += done[e];
    EXPECT(wh_reset(&cfg, B, state.data(), done.data(), nullptr, train, seed, 0, nullptr) == WH_OK);
    filled = filled < cap ? filled + 1 : cap;

    for (int64_t M : {(int64_t)1, 2 * B + 1, filled * B}) {
      std::vector<int64_t> idx(M), idx_out(M);
      for (int64_t m = 0; m < M; ++m) idx[m] = (int64_t)(rng() % (uint64_t)(filled * B));
      if (M > 1) idx[1] = idx[0];                                   // a duplicate
      if (M > 4) {                                                  // invalid entries
        idx[2] = -1;
        idx[3] = filled * B;
        idx[4] = (int64_t)1 << 62;
      }
      std::vector<float> obs((size_t)M * NA * OBS), nobs((size_t)M * NA * OBS), rw((size_t)M * NA);
      std::vector<uint32_t> st((size_t)W * M), nst((size_t)W * M);
      std::vector<int32_t> ac((size_t)M * NA), n(M);
      std::vector<uint8_t> dn(M);
      const wh_replay_batch all{obs.data(), nobs.data(), nullptr, nullptr, st.data(), nst.data(), ac.data(),
                                rw.data(),  dn.data(),   n.data(), idx_out.data()};
      EXPECT(wh_replay_gather(&cfg, B, &ring, filled, M, idx.data(), seed, 0, &all, nullptr) == WH_OK);
      for (int64_t m = 0; m < M; ++m) {
        const bool ok = idx[m] >= 0 && idx[m] < filled * B;
        EXPECT(ok ? (n[m] >= 1 && n[m] <= NA && idx_out[m] == idx[m]) : (n[m] == -1 && idx_out[m] == 0));
        if (!ok) {
          for (int k = 0; k < NA * OBS; ++k) EXPECT(obs[m * NA * OBS + k] == 0.0f && nobs[m * NA * OBS + k] == 0.0f);
          for (int w = 0; w < W; ++w) EXPECT(st[(size_t)w * M + m] == 0u && nst[(size_t)w * M + m] == 0u);
        } else {
          EXPECT(obs[m * NA * OBS] == (float)n[m]);                 // feature 0 of row 0: num_agents
          // the state copy observes to the same rows
          std::vector<float> again((size_t)NA * OBS);
          std::vector<uint32_t> one(W);
          for (int w = 0; w < W; ++w) one[w] = nst[(size_t)w * M + m];
          EXPECT(wh_observe(&cfg, 1, one.data(), again.data(), nullptr) == WH_OK);
          EXPECT(!memcmp(again.data(), &nobs[m * NA * OBS], sizeof(float) * NA * OBS));
        }
      }
      if (M > 1) EXPECT(!memcmp(&obs[0], &obs[(size_t)NA * OBS], sizeof(float) * NA * OBS));
      // drawn indices, one output at a time (every other pointer NULL)
      std::vector<int64_t> drawn(M);
      const wh_replay_batch only_idx{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                     nullptr, nullptr, nullptr, drawn.data()};
      EXPECT(wh_replay_gather(&cfg, B, &ring, filled, M, nullptr, seed, (uint64_t)s << 33 | 5u, &only_idx, nullptr) == WH_OK);
      for (int64_t m = 0; m < M; ++m) EXPECT(drawn[m] >= 0 && drawn[m] < filled * B);
      const wh_replay_batch only_next{nullptr, nobs.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                                      nullptr, nullptr,     nullptr, nullptr};
      EXPECT(wh_replay_gather(&cfg, B, &ring, filled, M, drawn.data(), seed, 0, &only_next, nullptr) == WH_OK);
    }
  }
  EXPECT(dones_seen > 0);
  // refusals and empty calls touch nothing (NULL buffers would fault)
  const wh_replay_ring none{nullptr, nullptr, nullptr, nullptr, cap};
  int32_t n1 = 7;
  const wh_replay_batch bn{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n1, nullptr};
  EXPECT(wh_replay_gather(&cfg, B, &none, 1, 0, nullptr, 0, 0, &bn, nullptr) == WH_OK);
  EXPECT(wh_replay_gather(&cfg, 0, &none, 1, 4, nullptr, 0, 0, &bn, nullptr) == WH_OK);
  EXPECT(wh_replay_gather(&cfg, B, &none, 1, 1, nullptr, 0, 0, &bn, nullptr) == WH_EINVAL);
  EXPECT(wh_replay_gather(&cfg, B, &ring, cap + 1, 1, nullptr, 0, 0, &bn, nullptr) == WH_EINVAL);
  EXPECT(wh_replay_put(&cfg, 0, &none, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == WH_OK);
  EXPECT(wh_replay_put(&cfg, B, &ring, cap, 0, state.data(), acts.data(), nullptr, nullptr, nullptr) == WH_EINVAL);
  EXPECT(wh_replay_put(&cfg, B, &ring, 0, 2, state.data(), acts.data(), rew.data(), done.data(), nullptr) == WH_EINVAL);
  alignas(16) char frag[16];
  const wh_replay_batch bf{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n1, nullptr};
  wh_replay_batch bx = bf;
  bx.xfrag = frag;
  EXPECT(wh_replay_gather(&cfg, B, &ring, 1, 1, nullptr, 0, 0, &bx, nullptr) == WH_ENOTSUP);
  EXPECT(n1 == 7);
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
  printf("ASAN REPLAY OK\n");
  return 0;
}
