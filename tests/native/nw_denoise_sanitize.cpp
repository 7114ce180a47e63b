// nw_denoise_sanitize.cpp — the host-only code of the denoiser (rt_nw_adapt_variance, rt_nw_denoise_params_default /
// _check; rtmi_nw_scene.cpp) under AddressSanitizer and UBSan: a program of its own (`make asan-denoise`), nothing
// is preloaded.  Exact-size heap arrays, so a read or write one element past an end is reported.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <memory>

#include "../../include/rtmi_nw.h"

static int failures = 0;
#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                \
    }                                                            \
  } while (0)

int main() {
  for (int W = 1; W <= 9; W += 4)
    for (int H = 1; H <= 5; H += 2) {
      const size_t n = size_t(W) * H;
      std::unique_ptr<int64_t[]> sum(new int64_t[n * 3]);
      std::unique_ptr<uint64_t[]> m2(new uint64_t[n]);
      std::unique_ptr<int32_t[]> cnt(new int32_t[n]);
      std::unique_ptr<float[]> var(new float[n]);
      for (size_t p = 0; p < n; ++p) {
        cnt[p] = int32_t(p % 5);  // 0 and 1 among them
        for (int c = 0; c < 3; ++c) sum[3 * p + c] = int64_t(p + 1) * cnt[p] * (int64_t(1) << 30);
        m2[p] = p % 3 == 0 ? std::numeric_limits<uint64_t>::max() : uint64_t(cnt[p]) * (p + 1) * (p + 1) * 9 * (uint64_t(1) << 24);
      }
      CHECK(rt_nw_adapt_variance(sum.get(), m2.get(), cnt.get(), W, H, var.get()) == 0);
      for (size_t p = 0; p < n; ++p) CHECK(cnt[p] < 2 ? std::isinf(var[p]) && var[p] > 0 : std::isfinite(var[p]) && var[p] >= 0);
      CHECK(rt_nw_adapt_variance(nullptr, m2.get(), cnt.get(), W, H, var.get()) == RT_EINVAL);
      CHECK(rt_nw_adapt_variance(sum.get(), m2.get(), cnt.get(), W, H, nullptr) == RT_EINVAL);
      CHECK(rt_nw_adapt_variance(sum.get(), m2.get(), cnt.get(), 0, H, var.get()) == RT_EINVAL);
      cnt[n - 1] = -1;
      CHECK(rt_nw_adapt_variance(sum.get(), m2.get(), cnt.get(), W, H, var.get()) == RT_EINVAL);
    }
  rt_nw_denoise_params p;
  CHECK(rt_nw_denoise_params_default(&p) == 0);
  CHECK(p.iterations == 5 && p.sigma_l == 4.0f && p.sigma_n == 128.0f && p.sigma_z == 1.0f && p.flags == RT_NW_DENOISE_DEMODULATE);
  CHECK(rt_nw_denoise_params_check(&p) == 0);
  CHECK(rt_nw_denoise_params_default(nullptr) == RT_EINVAL && rt_nw_denoise_params_check(nullptr) == RT_EINVAL);
  for (int it : {0, 9, -1}) {
    rt_nw_denoise_params q = p;
    q.iterations = it;
    CHECK(rt_nw_denoise_params_check(&q) == RT_EINVAL);
  }
  for (float bad : {0.0f, -1.0f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()})
    for (int which = 0; which < 3; ++which) {
      rt_nw_denoise_params q = p;
      (which == 0 ? q.sigma_l : which == 1 ? q.sigma_n : q.sigma_z) = bad;
      CHECK(rt_nw_denoise_params_check(&q) == RT_EINVAL);
    }
  rt_nw_denoise_params q = p;
  q.flags = 4;
  CHECK(rt_nw_denoise_params_check(&q) == RT_EINVAL);
  q.flags = RT_NW_DENOISE_DEMODULATE | RT_NW_DENOISE_NO_EDGES;
  CHECK(rt_nw_denoise_params_check(&q) == 0);
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
