// Stand-alone host check of the prediction-head C-ABI (bcnf_amd/csrc/bcnf_head.hip): the workspace plan and the
// argument validation, which return before any launch, so no GPU is needed. Built with the host side under
// AddressSanitizer + UBSan and run directly (tools/head_host_check.sh):
//   hipcc --offload-arch=gfx950 -std=c++17 -Iinclude -Xarch_host -fsanitize=address,undefined \
//         bcnf_amd/csrc/bcnf_head.hip tools/head_host_check.cpp -o build_exp/head_host_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "bcnf_amd.h"

static int fails = 0;
#define EXPECT(cond)                                                \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++fails;                                                      \
    }                                                               \
  } while (0)

int main() {
  // workspace: positive, 16-byte granular, at least the residual, non-decreasing in B, over a dense sweep of B
  // (every split-plan boundary) and the extremes of K and D
  const int Ks[] = {1, 3, 4, 37, 63, 64, 65, 128, 512, 1360, 1 << 20};
  const int Ds[] = {2, 3, 16, 17, 19, 21, 32};
  long long checked = 0;
  for (int K : Ks)
    for (int D : Ds) {
      int64_t prev = 0;
      for (int64_t B = 1; B <= 70000; B += (B < 5000 ? 1 : 997)) {
        int64_t n = -1;
        EXPECT(bcnf_head_work_bytes(B, K, D, &n) == BCNF_OK);
        EXPECT(n > 0 && n % 16 == 0 && n >= 4 * B * D && n >= prev);
        prev = n;
        ++checked;
      }
      int64_t n = -1;
      EXPECT(bcnf_head_work_bytes(INT32_MAX - 16, K, D, &n) == BCNF_OK && n > 0);
      EXPECT(bcnf_head_work_bytes(INT32_MAX, K, D, &n) == BCNF_ERR_ARG);
      EXPECT(bcnf_head_work_bytes(INT64_MAX, K, D, &n) == BCNF_ERR_ARG);
    }
  int64_t n = 0;
  EXPECT(bcnf_head_work_bytes(0, 8, 4, &n) == BCNF_ERR_ARG);
  EXPECT(bcnf_head_work_bytes(-5, 8, 4, &n) == BCNF_ERR_ARG);
  EXPECT(bcnf_head_work_bytes(8, 0, 4, &n) == BCNF_ERR_ARG);
  EXPECT(bcnf_head_work_bytes(8, -1, 4, &n) == BCNF_ERR_ARG);
  EXPECT(bcnf_head_work_bytes(8, INT32_MAX, 4, &n) == BCNF_ERR_ARG);
  EXPECT(bcnf_head_work_bytes(8, 8, 1, &n) == BCNF_ERR_ARG);
  EXPECT(bcnf_head_work_bytes(8, 8, 33, &n) == BCNF_ERR_ARG);
  EXPECT(bcnf_head_work_bytes(8, 8, 4, nullptr) == BCNF_ERR_ARG);

  // argument validation of the launching entry points: every call below must return BCNF_ERR_ARG without touching
  // its pointers (host memory here) or the HIP runtime
  float* buf = static_cast<float*>(std::aligned_alloc(64, 4096));
  float* odd = buf + 1;      // not 16-byte aligned
  EXPECT(bcnf_head_mse_forward(nullptr, 8, 8, buf, buf, buf, 4, 4, buf, nullptr) == BCNF_ERR_ARG);
  EXPECT(bcnf_head_mse_forward(buf, 8, 8, nullptr, buf, buf, 4, 4, buf, nullptr) == BCNF_ERR_ARG);
  EXPECT(bcnf_head_mse_forward(buf, 8, 8, buf, buf, nullptr, 4, 4, buf, nullptr) == BCNF_ERR_ARG);
  EXPECT(bcnf_head_mse_forward(buf, 8, 8, buf, buf, buf, 4, 4, nullptr, nullptr) == BCNF_ERR_ARG);
  EXPECT(bcnf_head_mse_forward(buf, 8, 8, buf, buf, buf, 4, 4, odd, nullptr) == BCNF_ERR_ARG);
  EXPECT(bcnf_head_mse_forward(buf, 7, 8, buf, buf, buf, 4, 4, buf, nullptr) == BCNF_ERR_ARG);
  EXPECT(bcnf_head_mse_forward(buf, 8, 0, buf, buf, buf, 4, 4, buf, nullptr) == BCNF_ERR_ARG);
  EXPECT(bcnf_head_mse_forward(buf, 8, 8, buf, buf, buf, 0, 4, buf, nullptr) == BCNF_ERR_ARG);
  EXPECT(bcnf_head_mse_forward(buf, 8, 8, buf, buf, buf, 4, 1, buf, nullptr) == BCNF_ERR_ARG);
  EXPECT(bcnf_head_mse_forward(buf, 8, 8, buf, buf, buf, 4, 33, buf, nullptr) == BCNF_ERR_ARG);
  EXPECT(bcnf_head_mse_backward(nullptr, 8, 8, buf, buf, nullptr, 1.f, 4, 4, buf, buf, buf, 8, 1, nullptr) ==
         BCNF_ERR_ARG);
  EXPECT(bcnf_head_mse_backward(buf, 8, 8, nullptr, buf, nullptr, 1.f, 4, 4, buf, buf, buf, 8, 1, nullptr) ==
         BCNF_ERR_ARG);
  EXPECT(bcnf_head_mse_backward(buf, 8, 8, buf, nullptr, nullptr, 1.f, 4, 4, buf, buf, buf, 8, 1, nullptr) ==
         BCNF_ERR_ARG);
  EXPECT(bcnf_head_mse_backward(buf, 7, 8, buf, buf, nullptr, 1.f, 4, 4, buf, buf, buf, 8, 1, nullptr) ==
         BCNF_ERR_ARG);
  EXPECT(bcnf_head_mse_backward(buf, 8, 8, buf, buf, nullptr, 1.f, 4, 4, buf, buf, buf, 7, 1, nullptr) ==
         BCNF_ERR_ARG);
  EXPECT(bcnf_head_mse_backward(buf, 8, 8, buf, buf, nullptr, -1.f, 4, 4, buf, buf, buf, 8, 1, nullptr) ==
         BCNF_ERR_ARG);
  EXPECT(bcnf_head_mse_backward(buf, 8, 8, buf, buf, nullptr, 1.f, 0, 4, buf, buf, buf, 8, 1, nullptr) ==
         BCNF_ERR_ARG);
  EXPECT(bcnf_head_mse_backward(buf, 8, 8, buf, buf, nullptr, 1.f, 4, 1, buf, buf, buf, 8, 1, nullptr) ==
         BCNF_ERR_ARG);
  EXPECT(bcnf_head_mse_backward(buf, 8, 8, buf, buf, nullptr, 1.f, 4, 33, buf, buf, buf, 8, 1, nullptr) ==
         BCNF_ERR_ARG);
  EXPECT(bcnf_hybrid_finalize(nullptr, buf, 4, 4, 1.f, nullptr, nullptr) == BCNF_ERR_ARG);
  EXPECT(bcnf_hybrid_finalize(buf, nullptr, 4, 4, 1.f, nullptr, nullptr) == BCNF_ERR_ARG);
  EXPECT(bcnf_hybrid_finalize(buf, buf, 0, 4, 1.f, nullptr, nullptr) == BCNF_ERR_ARG);
  EXPECT(bcnf_hybrid_finalize(buf, buf, 4, 33, 1.f, nullptr, nullptr) == BCNF_ERR_ARG);
  EXPECT(bcnf_hybrid_finalize(buf, buf, 4, 4, -1.f, nullptr, nullptr) == BCNF_ERR_ARG);
  std::free(buf);
  std::printf("head_host_check: %lld workspace plans checked, %d failures\n", checked, fails);
  return fails ? 1 : 0;
}
