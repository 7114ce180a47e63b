// nw_adaptive_sanitize.cpp — the host code of adaptive sampling (rtmi_nw_scene.cpp: rt_nw_adapt_criterion, the
// adaptive checkpoint file) under ASan + UBSan, a program of its own (`make asan-adaptive`,
// tests/test_nw_adaptive.py): the criterion on buffers at every edge of its index arithmetic, checkpoint files
// written, read back, cut short, lengthened and mislabelled.  Usage: nw_adaptive_sanitize WORKDIR (left empty).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../a_dive_into_ray_tracing_amd/csrc/rtmi_nw_internal.h"

using namespace rtmi::nw;

static int failures = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, rt_last_error()); \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

static void criterion_cases() {
  const int64_t one = int64_t(1) << 32;
  for (int W : {1, 2, 9, 64})
    for (int H : {1, 3, 17}) {
      const size_t np = size_t(W) * H;
      std::vector<int64_t> sum(np * 3);
      std::vector<uint64_t> m2(np);
      std::vector<int32_t> n(np);
      for (size_t p = 0; p < np; ++p) {
        n[p] = int32_t(p % 5 == 0 ? 0 : p % 7 == 0 ? RT_NW_ADAPT_MAX_SPP : 16 + p % 100);
        const uint64_t l = uint64_t(3 * (p % 64 + 1) * one) >> 18;
        for (int c = 0; c < 3; ++c) sum[3 * p + c] = int64_t(n[p]) * int64_t(p % 64 + 1) * one;
        m2[p] = uint64_t(n[p]) * l * l + (p % 3 ? uint64_t(n[p]) * l * (l / 4) : 0);  // up to 2^20 * (192 * 2^14)^2
      }
      std::vector<uint8_t> active(np, 7);
      std::vector<double> err(np, -1.0);
      for (int dilate : {0, 1, 3, 1000, 2147483647}) {
        int64_t count = -1;
        CHECK(rt_nw_adapt_criterion(sum.data(), m2.data(), n.data(), W, H, 16, RT_NW_ADAPT_MAX_SPP, 0.05, 0.03, dilate,
                                    active.data(), err.data(), &count) == RT_OK);
        int64_t seen = 0;
        for (size_t p = 0; p < np; ++p) {
          CHECK(active[p] <= 1);
          CHECK(!(n[p] >= RT_NW_ADAPT_MAX_SPP && active[p]));
          CHECK(n[p] >= 2 ? std::isfinite(err[p]) && err[p] >= 0 : std::isinf(err[p]));
          seen += active[p];
        }
        CHECK(seen == count);
      }
      CHECK(rt_nw_adapt_criterion(sum.data(), m2.data(), n.data(), W, H, 16, 256, 0.0, 0.03, 1, active.data(), nullptr, nullptr) == RT_OK);
      CHECK(rt_nw_adapt_criterion(sum.data(), m2.data(), n.data(), W, H, 16, 1, 0.05, 0.03, 1, active.data(), nullptr, nullptr) == RT_EINVAL);
      CHECK(rt_nw_adapt_criterion(sum.data(), m2.data(), n.data(), W, H, 16, 256, 0.05, 0.03, -1, active.data(), nullptr, nullptr) == RT_EINVAL);
    }
}

static bool write_file(const std::string &path, const std::vector<char> &bytes, size_t count) {
  FILE *f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(bytes.data(), 1, count, f) == count;
  return std::fclose(f) == 0 && ok;
}

static void checkpoint_cases(const std::string &dir) {
  const int32_t W = 5, rows = 3;
  const size_t np = size_t(W) * rows;
  std::vector<int64_t> sum(np * 3);
  std::vector<uint64_t> m2(np);
  std::vector<int32_t> n(np);
  for (size_t p = 0; p < np; ++p) {
    sum[3 * p] = int64_t(p) << 33;
    m2[p] = ~uint64_t(0) - p;
    n[p] = int32_t(p);
  }
  CkptHeader h{};
  h.W = W;
  h.H = 7;
  h.row0 = 1;
  h.row_step = 2;
  h.nrows = rows;
  h.spp_done = int32_t(np) - 1;
  h.max_depth = 50;
  h.seed = 1984;
  h.scene_hash = 0x0123456789abcdefull;
  h.camera_hash = 0xfedcba9876543210ull;
  const std::string good = dir + "/good.ckpt";
  CHECK(adapt_ckpt_write(good.c_str(), h, sum.data(), m2.data(), n.data()) == RT_OK);
  CkptHeader r{};
  std::vector<int64_t> rs;
  std::vector<uint64_t> rm;
  std::vector<int32_t> rn;
  CHECK(adapt_ckpt_read(good.c_str(), r, &rs, &rm, &rn) == RT_OK);
  CHECK(rs == sum && rm == m2 && rn == n && r.W == W && r.nrows == rows && r.seed == 1984 && std::memcmp(r.magic, "RTMINWD1", 8) == 0);
  int32_t v8[8];
  uint64_t v3[3];
  CHECK(rt_nw_adapt_info(good.c_str(), v8, v3) == RT_OK && v8[0] == W && v8[4] == rows && v8[5] == int32_t(np) - 1 && v3[1] == h.scene_hash);
  CHECK(rt_nw_accum_info(good.c_str(), v8, v3) == RT_EIO);  // no progressive checkpoint
  // the same bytes cut short, lengthened, mislabelled, and with a header that lies about the size
  FILE *f = std::fopen(good.c_str(), "rb");
  std::vector<char> bytes(64 + np * 36 + 8);
  const size_t len = f ? std::fread(bytes.data(), 1, bytes.size(), f) : 0;
  if (f) std::fclose(f);
  CHECK(len == 64 + np * 36);
  const std::string bad = dir + "/bad.ckpt";
  for (size_t cut : {size_t(0), size_t(7), size_t(63), size_t(64), len - 1, len + 1, len + 8}) {
    CHECK(write_file(bad, bytes, cut));
    CHECK(rt_nw_adapt_info(bad.c_str(), v8, v3) == RT_EIO);
    CHECK(adapt_ckpt_read(bad.c_str(), r, &rs, &rm, &rn) == RT_EIO);
  }
  std::vector<char> other = bytes;
  std::memcpy(other.data(), "RTMINWA1", 8);
  CHECK(write_file(bad, other, len) && rt_nw_adapt_info(bad.c_str(), v8, v3) == RT_EIO);
  for (int32_t w : {0, -5, 6, 2147483647}) {
    other = bytes;
    std::memcpy(other.data() + 8, &w, 4);
    CHECK(write_file(bad, other, len) && rt_nw_adapt_info(bad.c_str(), v8, v3) == RT_EIO);
  }
  CHECK(rt_nw_adapt_info((dir + "/missing.ckpt").c_str(), v8, v3) == RT_EIO);
  CHECK(adapt_ckpt_write((dir + "/no/such/dir.ckpt").c_str(), h, sum.data(), m2.data(), n.data()) == RT_EIO);
  std::remove(good.c_str());
  std::remove(bad.c_str());
}

int main(int argc, char **argv) {
  if (argc != 2) {
    std::printf("usage: %s WORKDIR\n", argv[0]);
    return 2;
  }
  criterion_cases();
  checkpoint_cases(argv[1]);
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
