// The argument front end of the MLP training entry points (csrc/abi_args.h: mlp_train_query_call,
// mlp_train_forward_call, mlp_backward_call) under AddressSanitizer + UndefinedBehaviorSanitizer: the
// desc and the two pointer structs are heap objects of exactly their size, so a read past one is
// reported, and every rule of include/warehouse_amd.h (MLP TRAINING) is asked in the header's order.
// The front end dereferences d, w and g only: every other pointer is a dummy.  Built and run by
// tests/test_asan_mlp_train.py; prints "ASAN MLP TRAIN OK" on a clean run.
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

int fwd(const wh_mlp_desc* d, const wh_mlp_weights* w, int64_t rows, uintptr_t obs = 0x1000, uintptr_t h0 = 0x2000,
        uintptr_t h1 = 0x3000, uintptr_t lg = 0x4000, bool* live = nullptr) {
  bool l;
  return wh_abi::mlp_train_forward_call(d, w, rows, fp(obs), fp(h0), fp(h1), fp(lg), live ? live : &l);
}

int bwd(const wh_mlp_desc* d, const wh_mlp_weights* w, int64_t rows, const wh_mlp_grads* g, uintptr_t work = 0x6000,
        uintptr_t obs = 0x1000, uintptr_t dz = 0x5000) {
  return wh_abi::mlp_backward_call(d, w, rows, fp(obs), fp(0x2000), fp(0x3000), fp(dz), g, reinterpret_cast<void*>(work));
}

}  // namespace

int main() {
  const int32_t shapes[3][3] = {{37, 256, 256}, {82, 512, 512}, {145, 1024, 256}};
  for (const auto& s : shapes) {
    auto d = std::make_unique<wh_mlp_desc>(wh_mlp_desc{s[0], s[1], s[2], 9, WH_MLP_F32});
    auto w = std::make_unique<wh_mlp_weights>(wh_mlp_weights{fp(0x10), fp(0x20), fp(0x30), fp(0x40), fp(0x50), fp(0x60)});
    auto g = std::make_unique<wh_mlp_grads>(wh_mlp_grads{fpm(0x110), fpm(0x120), fpm(0x130), fpm(0x140), fpm(0x150), fpm(0x160)});
    bool live = true;
    EXPECT(wh_abi::mlp_train_query_call(d.get(), 0) == WH_OK && wh_abi::mlp_train_query_call(d.get(), WH_MLP_TRAIN_MAX_ROWS) == WH_OK);
    EXPECT(wh_abi::mlp_train_query_call(d.get(), -1) == WH_EINVAL);
    EXPECT(wh_abi::mlp_train_query_call(d.get(), (int64_t)WH_MLP_TRAIN_MAX_ROWS + 1) == WH_EINVAL);
    EXPECT(wh_abi::mlp_train_query_call(nullptr, 5) == WH_EINVAL);
    EXPECT(fwd(d.get(), w.get(), 5, 0x1000, 0x2000, 0x3000, 0x4000, &live) == WH_OK && live);
    EXPECT(fwd(d.get(), w.get(), 0, 0x1000, 0x2000, 0x3000, 0x4000, &live) == WH_OK && !live);
    EXPECT(bwd(d.get(), w.get(), 5, g.get()) == WH_OK && bwd(d.get(), w.get(), 0, g.get()) == WH_OK);
    EXPECT(fwd(nullptr, nullptr, -1) == WH_EINVAL && bwd(nullptr, nullptr, -1, nullptr, 1) == WH_EINVAL);
    for (int k = 0; k < 5; ++k) {   // a wrong shape, out_dim or precision answers before rows and every pointer
      auto b = std::make_unique<wh_mlp_desc>(*d);
      if (k == 0) b->in_dim += 1;
      if (k == 1) b->hidden0 /= 2;
      if (k == 2) b->hidden1 *= 2;
      if (k == 3) b->out_dim = 8;
      if (k == 4) b->precision = WH_MLP_BF16;
      EXPECT(wh_abi::mlp_train_query_call(b.get(), -1) == WH_ENOTSUP);
      EXPECT(fwd(b.get(), nullptr, -1, 0) == WH_ENOTSUP && bwd(b.get(), nullptr, -1, nullptr, 1) == WH_ENOTSUP);
    }
    EXPECT(fwd(d.get(), nullptr, -1, 0) == WH_EINVAL && bwd(d.get(), nullptr, -1, nullptr, 1) == WH_EINVAL);
    for (int64_t rows : {(int64_t)5, (int64_t)0}) {
      EXPECT(fwd(d.get(), nullptr, rows) == WH_EINVAL && bwd(d.get(), nullptr, rows, g.get()) == WH_EINVAL);
      EXPECT(bwd(d.get(), w.get(), rows, nullptr) == WH_EINVAL);
      for (int k = 0; k < 6; ++k) {
        auto bw = std::make_unique<wh_mlp_weights>(*w);
        auto bg = std::make_unique<wh_mlp_grads>(*g);
        (&bw->w0)[k] = nullptr;
        (&bg->w0)[k] = nullptr;
        EXPECT(fwd(d.get(), bw.get(), rows) == WH_EINVAL && bwd(d.get(), bw.get(), rows, g.get()) == WH_EINVAL);
        EXPECT(bwd(d.get(), w.get(), rows, bg.get()) == WH_EINVAL);
      }
      EXPECT(fwd(d.get(), w.get(), rows, 0) == WH_EINVAL && fwd(d.get(), w.get(), rows, 0x1000, 0) == WH_EINVAL);
      EXPECT(fwd(d.get(), w.get(), rows, 0x1000, 0x2000, 0) == WH_EINVAL);
      EXPECT(fwd(d.get(), w.get(), rows, 0x1000, 0x2000, 0x3000, 0) == WH_EINVAL);
      EXPECT(bwd(d.get(), w.get(), rows, g.get(), 0) == WH_EINVAL && bwd(d.get(), w.get(), rows, g.get(), 0x6008) == WH_EINVAL);
      EXPECT(bwd(d.get(), w.get(), rows, g.get(), 0x6000, 0) == WH_EINVAL);
      EXPECT(bwd(d.get(), w.get(), rows, g.get(), 0x6000, 0x1000, 0) == WH_EINVAL);
    }
    EXPECT(fwd(d.get(), w.get(), (int64_t)WH_MLP_TRAIN_MAX_ROWS + 1) == WH_EINVAL);
    EXPECT(bwd(d.get(), w.get(), (int64_t)WH_MLP_TRAIN_MAX_ROWS + 1, g.get()) == WH_EINVAL);
    EXPECT(fwd(d.get(), w.get(), WH_MLP_TRAIN_MAX_ROWS) == WH_OK && bwd(d.get(), w.get(), WH_MLP_TRAIN_MAX_ROWS, g.get()) == WH_OK);
  }
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("ASAN MLP TRAIN OK\n");
  return 0;
}
