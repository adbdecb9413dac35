// The argument front end of the multi-network training entry points (csrc/abi_args.h:
// mlp_train_multi_call) under AddressSanitizer + UndefinedBehaviorSanitizer.  The job array is a heap
// array of exactly `nnets` elements, so a check that reads job `nnets` is reported; every rule of
// include/warehouse_amd.h (MLP TRAINING, the multi calls) is asked in the header's order, each case
// breaking two rules and expecting the code of the earlier one where the codes differ.  The front end
// dereferences d and the jobs only: every other pointer is a dummy.  Built and run by
// tests/test_asan_mlp_train_multi.py; prints "ASAN MLP TRAIN MULTI OK" on a clean run.
#include <stdint.h>
#include <stdio.h>

#include <memory>

#include "abi_args.h"

namespace {

int fails = 0;
#define EXPECT(c)                                                  \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                     \
    }                                                              \
  } while (0)

const float* fp(uintptr_t v) { return reinterpret_cast<const float*>(v); }
float* fpm(uintptr_t v) { return reinterpret_cast<float*>(v); }

// job i with every pointer its own (obs shared by all jobs, which is allowed)
wh_mlp_train_job good(int i) {
  const uintptr_t b = 0x100000 * (uintptr_t)(i + 1);
  wh_mlp_train_job j{};
  j.w = wh_mlp_weights{fp(b + 0x10), fp(b + 0x20), fp(b + 0x30), fp(b + 0x40), fp(b + 0x50), fp(b + 0x60)};
  j.obs = fp(0x1000);
  j.h0 = fpm(b + 0x1000);
  j.h1 = fpm(b + 0x2000);
  j.logits = fpm(b + 0x3000);
  j.dlogits = fp(b + 0x4000);
  j.g = wh_mlp_grads{fpm(b + 0x5010), fpm(b + 0x5020), fpm(b + 0x5030), fpm(b + 0x5040), fpm(b + 0x5050), fpm(b + 0x5060)};
  j.work = reinterpret_cast<void*>(b + 0x6000);
  return j;
}

std::unique_ptr<wh_mlp_train_job[]> jobs_of(int n) {
  std::unique_ptr<wh_mlp_train_job[]> a(new wh_mlp_train_job[n]);
  for (int i = 0; i < n; ++i) a[i] = good(i);
  return a;
}

int call(const wh_mlp_desc* d, int32_t n, const wh_mlp_train_job* jobs, int64_t rows, bool backward) {
  return wh_abi::mlp_train_multi_call(d, n, jobs, rows, backward);
}

}  // namespace

int main() {
  const int32_t shapes[3][3] = {{37, 256, 256}, {82, 512, 512}, {145, 1024, 256}};
  const int64_t OVER = (int64_t)WH_MLP_TRAIN_MAX_ROWS + 1;
  for (const auto& s : shapes) {
    auto d = std::make_unique<wh_mlp_desc>(wh_mlp_desc{s[0], s[1], s[2], 9, WH_MLP_F32});
    for (int dir = 0; dir < 2; ++dir) {
      const bool bw = dir == 1;
      // what is accepted: every count of jobs, the empty batch, the largest one, no job at all
      for (int n = 0; n <= WH_MLP_TRAIN_MAX_NETS; ++n) {
        auto a = jobs_of(n);
        for (int64_t rows : {(int64_t)5, (int64_t)0, (int64_t)WH_MLP_TRAIN_MAX_ROWS}) EXPECT(call(d.get(), n, a.get(), rows, bw) == WH_OK);
      }
      EXPECT(call(d.get(), 0, nullptr, 5, bw) == WH_OK);
      // the fields of the other direction are not looked at
      {
        auto a = jobs_of(2);
        if (bw) a[0].logits = a[1].logits = nullptr;
        else {
          a[0].dlogits = nullptr; a[0].g = wh_mlp_grads{}; a[0].work = nullptr;
          a[1].dlogits = nullptr; a[1].g = wh_mlp_grads{}; a[1].work = reinterpret_cast<void*>((uintptr_t)3);
        }
        EXPECT(call(d.get(), 2, a.get(), 5, bw) == WH_OK);
      }
      auto two = jobs_of(2);
      // d == NULL, before the shape (there is none), rows, the count and the jobs
      EXPECT(call(nullptr, 2, two.get(), 5, bw) == WH_EINVAL);
      EXPECT(call(nullptr, -1, nullptr, -1, bw) == WH_EINVAL);
      // a wrong shape, out_dim or precision: before rows, the count and every job
      for (int k = 0; k < 6; ++k) {
        auto b = std::make_unique<wh_mlp_desc>(*d);
        if (k == 0) b->in_dim += 1;
        if (k == 1) b->hidden0 /= 2;
        if (k == 2) b->hidden1 *= 2;
        if (k == 3) b->out_dim = 8;
        if (k == 4) b->precision = WH_MLP_BF16;
        if (k == 5) b->precision = 7;
        EXPECT(call(b.get(), 2, two.get(), 5, bw) == WH_ENOTSUP);
        EXPECT(call(b.get(), 2, two.get(), -1, bw) == WH_ENOTSUP);
        EXPECT(call(b.get(), 2, two.get(), OVER, bw) == WH_ENOTSUP);
        EXPECT(call(b.get(), WH_MLP_TRAIN_MAX_NETS + 1, nullptr, 5, bw) == WH_ENOTSUP);
        EXPECT(call(b.get(), -1, nullptr, -1, bw) == WH_ENOTSUP);
      }
      // rows: before the count (a NULL array of too many jobs is never read) and every job
      for (int64_t rows : {(int64_t)-1, OVER}) {
        EXPECT(call(d.get(), 2, two.get(), rows, bw) == WH_EINVAL);
        EXPECT(call(d.get(), WH_MLP_TRAIN_MAX_NETS + 1, nullptr, rows, bw) == WH_EINVAL);
        EXPECT(call(d.get(), 0, nullptr, rows, bw) == WH_EINVAL);
      }
      // the count: before any job is read (the array is shorter than the count says)
      EXPECT(call(d.get(), -1, two.get(), 5, bw) == WH_EINVAL);
      EXPECT(call(d.get(), WH_MLP_TRAIN_MAX_NETS + 1, two.get(), 5, bw) == WH_EINVAL);
      EXPECT(call(d.get(), 1, nullptr, 5, bw) == WH_EINVAL);
      EXPECT(call(d.get(), WH_MLP_TRAIN_MAX_NETS, nullptr, 0, bw) == WH_EINVAL);
      // every job's own pointers, in every position, also for the empty batch
      for (int n = 1; n <= WH_MLP_TRAIN_MAX_NETS; ++n)
        for (int at = 0; at < n; ++at)
          for (int64_t rows : {(int64_t)5, (int64_t)0}) {
            for (int k = 0; k < 6; ++k) {
              auto a = jobs_of(n);
              (&a[at].w.w0)[k] = nullptr;
              EXPECT(call(d.get(), n, a.get(), rows, bw) == WH_EINVAL);
              if (bw) {
                a = jobs_of(n);
                (&a[at].g.w0)[k] = nullptr;
                EXPECT(call(d.get(), n, a.get(), rows, bw) == WH_EINVAL);
              }
            }
            for (int k = 0; k < 3; ++k) {
              auto a = jobs_of(n);
              if (k == 0) a[at].obs = nullptr;
              if (k == 1) a[at].h0 = nullptr;
              if (k == 2) a[at].h1 = nullptr;
              EXPECT(call(d.get(), n, a.get(), rows, bw) == WH_EINVAL);
            }
            auto a = jobs_of(n);
            if (bw) a[at].dlogits = nullptr; else a[at].logits = nullptr;
            EXPECT(call(d.get(), n, a.get(), rows, bw) == WH_EINVAL);
            if (bw) {
              for (uintptr_t off : {(uintptr_t)1, (uintptr_t)4, (uintptr_t)8}) {
                a = jobs_of(n);
                a[at].work = reinterpret_cast<void*>((uintptr_t)a[at].work + off);
                EXPECT(call(d.get(), n, a.get(), rows, bw) == WH_EINVAL);
              }
              a = jobs_of(n);
              a[at].work = nullptr;
              EXPECT(call(d.get(), n, a.get(), rows, bw) == WH_EINVAL);
            }
          }
      // two jobs that would write one buffer: every pair, every field
      for (int n = 2; n <= WH_MLP_TRAIN_MAX_NETS; ++n)
        for (int hi = 1; hi < n; ++hi)
          for (int lo = 0; lo < hi; ++lo) {
            if (!bw) {
              for (int k = 0; k < 3; ++k) {
                auto a = jobs_of(n);
                if (k == 0) a[hi].h0 = a[lo].h0;
                if (k == 1) a[hi].h1 = a[lo].h1;
                if (k == 2) a[hi].logits = a[lo].logits;
                EXPECT(call(d.get(), n, a.get(), 5, bw) == WH_EINVAL);
                EXPECT(call(d.get(), n, a.get(), 0, bw) == WH_EINVAL);
              }
            } else {
              for (int k = 0; k < 6; ++k) {
                auto a = jobs_of(n);
                (&a[hi].g.w0)[k] = (&a[lo].g.w0)[k];
                EXPECT(call(d.get(), n, a.get(), 5, bw) == WH_EINVAL);
                EXPECT(call(d.get(), n, a.get(), 0, bw) == WH_EINVAL);
              }
              auto a = jobs_of(n);
              a[hi].work = a[lo].work;
              EXPECT(call(d.get(), n, a.get(), 5, bw) == WH_EINVAL);
            }
            // shared inputs are no defect: one obs, one set of weights, (backward) one dlogits
            auto a = jobs_of(n);
            a[hi].obs = a[lo].obs;
            a[hi].w = a[lo].w;
            a[hi].dlogits = a[lo].dlogits;
            if (bw) { a[hi].logits = a[lo].logits; a[hi].h0 = a[lo].h0; a[hi].h1 = a[lo].h1; }
            else { a[hi].g = a[lo].g; a[hi].work = a[lo].work; }
            EXPECT(call(d.get(), n, a.get(), 5, bw) == WH_OK);
          }
    }
  }
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("ASAN MLP TRAIN MULTI OK\n");
  return 0;
}
