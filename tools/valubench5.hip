// tools/valubench5.hip — cost of the root acceptance (rtmi_path.h resolve_root,
// resolve_key) and of the one-layer DDA step (hit_world_grid<.., FLAT_Y>) as
// whole dependent sequences, in C++ as the header writes them: the two-root
// acceptance against the one-root form of rtmi_accept.h (its `in` test by two
// float compares, and by one unsigned compare of offset bit patterns), and the
// step by selects against the step that recomputes both face parameters from
// their counters.  The acceptances start from hb, sqrt(disc) and 1/a (the root
// itself is tools/valubench4.hip's subject); the steps run without the loop's
// exit (the leave flag is accumulated instead).  8 independent chains per lane,
// 8 waves per SIMD, as tools/valubench4.hip.  One JSON line per form: cycles
// per sequence per SIMD.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o tools/valubench5_bin tools/valubench5.hip
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

enum Form { FMA, ROOT_TWO, ROOT_ONE, ROOT_ONE_BITS, KEY_TWO, KEY_ONE, KEY_ONE_BITS, STEP_SELECT, STEP_RECOMPUTE, NFORMS };

__shared__ uint16_t idx_tab[256];

struct Hit { float t_max; int32_t best; };

// ---- the acceptances ------------------------------------------------------------
template <bool KEY> __device__ __forceinline__ bool later_of(int32_t idx, int32_t best) {
  if constexpr (KEY) return (best < 0) | (idx_tab[idx & 255] > idx_tab[(best < 0 ? idx : best) & 255]);
  else return idx > best;
}
// today's: both roots accepted separately (resolve_root forms `later` on every call, resolve_key in the tie branch)
template <bool KEY> __device__ __forceinline__ void accept_two(int32_t idx, float hb, float sq, float inv_a, Hit &h) {
  const float r1 = (-hb - sq) * inv_a, r2 = (-hb + sq) * inv_a;
  bool ok1, ok2;
  if constexpr (!KEY) {
    const bool later = idx > h.best;
    ok1 = !(r1 < 0.001f) & ((r1 < h.t_max) | ((r1 == h.t_max) & later));
    ok2 = !(r2 < 0.001f) & ((r2 < h.t_max) | ((r2 == h.t_max) & later));
  } else {
    const bool g1 = !(r1 < 0.001f), g2 = !(r2 < 0.001f);
    ok1 = g1 & (r1 < h.t_max), ok2 = g2 & (r2 < h.t_max);
    const bool e1 = g1 & (r1 == h.t_max), e2 = g2 & (r2 == h.t_max);
    if (__builtin_expect(e1 | e2, 0)) {
      const bool later = later_of<true>(idx, h.best);
      ok1 |= e1 & later;
      ok2 |= e2 & later;
    }
  }
  if (ok1 || ok2) {
    h.t_max = ok1 ? r1 : r2;
    h.best = idx;
  }
}
// one selected root (rtmi_accept.h accept_root), BITS: `in` by one unsigned compare
template <bool KEY, bool BITS> __device__ __forceinline__ void accept_one(int32_t idx, float hb, float sq, float inv_a, Hit &h) {
  const float r1 = (-hb - sq) * inv_a, r2 = (-hb + sq) * inv_a;
  const float t = r1 >= 0.001f ? r1 : r2;
  bool ok;
  if constexpr (BITS) ok = (__float_as_uint(t) - 0x3A83126Fu) < (__float_as_uint(h.t_max) - 0x3A83126Fu);
  else ok = !(t < 0.001f) & (t < h.t_max);
  if (__builtin_expect(t == h.t_max, 0)) ok = later_of<KEY>(idx, h.best);
  if (ok) {
    h.t_max = t;
    h.best = idx;
  }
}

// ---- the one-layer step ------------------------------------------------------------
struct Walk { float kx, kz, tnx, tnz; uint32_t cell; };
struct Ray { float t0x, t0z, dtx, dtz, kmx, kmz, tny, t_max; int dcx, dcz; };

__device__ __forceinline__ bool step_select(Walk &w, const Ray &r) {
  const float texit = __builtin_fminf(w.tnx, __builtin_fminf(r.tny, w.tnz));
  const bool sx = (w.tnx <= r.tny) & (w.tnx <= w.tnz);
  const bool sy = !sx & (r.tny <= w.tnz);
  const bool leave = !(texit < r.t_max) | sy | ((sx ? w.kx : w.kz) >= (sx ? r.kmx : r.kmz));
  w.kx = sx ? w.kx + 1.0f : w.kx;
  w.kz = sx ? w.kz : w.kz + 1.0f;
  w.tnx = sx ? __builtin_fmaf(w.kx, r.dtx, r.t0x) : w.tnx;
  w.tnz = sx ? w.tnz : __builtin_fmaf(w.kz, r.dtz, r.t0z);
  w.cell += sx ? r.dcx : r.dcz;
  return leave;
}
__device__ __forceinline__ bool step_recompute(Walk &w, const Ray &r) {
  const float texit = __builtin_fminf(w.tnx, __builtin_fminf(r.tny, w.tnz));
  const bool sx = (w.tnx <= r.tny) & (w.tnx <= w.tnz);
  const bool sy = !sx & (r.tny <= w.tnz);
  const float sxf = sx ? 1.0f : 0.0f;
  w.kx += sxf;
  w.kz += 1.0f - sxf;
  w.tnx = __builtin_fmaf(w.kx, r.dtx, r.t0x);
  w.tnz = __builtin_fmaf(w.kz, r.dtz, r.t0z);
  w.cell += sx ? r.dcx : r.dcz;
  return !(texit < r.t_max) | sy | (w.kx > r.kmx) | (w.kz > r.kmz);
}

template <int MODE>
__global__ __launch_bounds__(256) void k(float *out, int iters, float scale) {
  idx_tab[threadIdx.x] = uint16_t(threadIdx.x * 7u);
  __syncthreads();
  const float lane = float(threadIdx.x);
  float acc = 0.0f;
  if constexpr (MODE == FMA) {
    float x0 = lane + 1, x1 = x0 + 1, x2 = x0 + 2, x3 = x0 + 3, x4 = x0 + 4, x5 = x0 + 5, x6 = x0 + 6, x7 = x0 + 7;
    const float va = 1.0000001f + lane * 1e-12f, vb = 1e-7f;
    for (int i = 0; i < iters; i++) {
#pragma unroll
      for (int r = 0; r < 8; r++) {
#define F_FMA(x) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(x) : "v"(vb), "v"(va));
        F_FMA(x0) F_FMA(x1) F_FMA(x2) F_FMA(x3) F_FMA(x4) F_FMA(x5) F_FMA(x6) F_FMA(x7)
      }
    }
    acc = x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7;
  } else if constexpr (MODE <= KEY_ONE_BITS) {
    // roots that wander around the held t_max: hb falls slowly, so that a chain accepts now and then
    Hit h[8];
    float hb[8];
    for (int c = 0; c < 8; c++) {
      h[c] = {__builtin_inff(), -1};
      hb[c] = -(2.0f + 0.01f * lane + c) * scale;
    }
    const float sq = 0.5f * scale + 1e-3f * lane, inv_a = 1.0f / scale, dhb = 1e-4f * scale;
    for (int i = 0; i < iters; i++) {
#pragma unroll
      for (int r = 0; r < 8; r++) {
#pragma unroll
        for (int c = 0; c < 8; c++) {
          const int32_t idx = (i * 8 + r) ^ c;
          if constexpr (MODE == ROOT_TWO) accept_two<false>(idx, hb[c], sq, inv_a, h[c]);
          else if constexpr (MODE == ROOT_ONE) accept_one<false, false>(idx, hb[c], sq, inv_a, h[c]);
          else if constexpr (MODE == ROOT_ONE_BITS) accept_one<false, true>(idx, hb[c], sq, inv_a, h[c]);
          else if constexpr (MODE == KEY_TWO) accept_two<true>(idx, hb[c], sq, inv_a, h[c]);
          else if constexpr (MODE == KEY_ONE) accept_one<true, false>(idx, hb[c], sq, inv_a, h[c]);
          else accept_one<true, true>(idx, hb[c], sq, inv_a, h[c]);
          // the next candidate's hb: a little nearer on odd rounds, farther on even ones (one v_fma_f32 per call,
          // the same in every form)
          hb[c] = __builtin_fmaf(dhb, (r & 1) ? 3.0f : -2.0f, hb[c]);
        }
      }
    }
    for (int c = 0; c < 8; c++) acc += h[c].t_max + float(h[c].best);
  } else {
    Walk w[8];
    Ray ry;
    ry = {0.3f * scale + 1e-3f * lane, 0.4f * scale + 2e-3f * lane, 0.7f * scale, 0.9f * scale + 1e-3f * lane,
          1e30f * scale, 1e30f * scale, 3e38f * scale, 2e38f * scale, threadIdx.x & 1 ? 4 : -4, threadIdx.x & 2 ? 80 : -80};
    for (int c = 0; c < 8; c++) w[c] = {0.0f, 0.0f, ry.t0x + c, ry.t0z + 0.5f * c, uint32_t(c)};
    unsigned left = 0;
    for (int i = 0; i < iters; i++) {
#pragma unroll
      for (int r = 0; r < 8; r++) {
#pragma unroll
        for (int c = 0; c < 8; c++) {
          if constexpr (MODE == STEP_SELECT) left += step_select(w[c], ry);
          else left += step_recompute(w[c], ry);
        }
      }
    }
    for (int c = 0; c < 8; c++) acc += w[c].kx + w[c].kz + w[c].tnx + w[c].tnz + float(w[c].cell);
    acc += float(left);
  }
  if (acc == 12345.f) out[0] = acc;
}

int main() {
  float *out;
  if (hipMalloc(&out, 4) != hipSuccess) {
    fprintf(stderr, "no device\n");
    return 1;
  }
  // 256 CUs x 4 SIMDs x 8 waves, 4 rounds of them
  const int blocks = 256 * 8 * 4, threads = 256, iters = 1000;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  const char *names[NFORMS] = {"v_fma_f32 v,v,v,v",
                               "resolve_root: two roots (parent)",
                               "resolve_root: one root, float in-test",
                               "resolve_root: one root, unsigned in-test",
                               "resolve_key: two roots (parent)",
                               "resolve_key: one root, float in-test",
                               "resolve_key: one root, unsigned in-test",
                               "one-layer step: selects (parent)",
                               "one-layer step: both faces recomputed"};
  void (*kern[NFORMS])(float *, int, float) = {k<0>, k<1>, k<2>, k<3>, k<4>, k<5>, k<6>, k<7>, k<8>};
  int clock_khz = 0;
  (void)hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeClockRate, 0);
  const double hz = clock_khz > 0 ? clock_khz * 1e3 : 2.4e9;
  int cus = 0;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
  const double simds = 4.0 * (cus > 0 ? cus : 256);
  double fma_cyc = 0;
  for (int m = 0; m < NFORMS; m++) {
    float best = 1e30f;
    for (int rep = 0; rep < 3; rep++) {
      (void)hipEventRecord(e0);
      hipLaunchKernelGGL(kern[m], dim3(blocks), dim3(threads), 0, 0, out, iters, 1.0f);
      (void)hipEventRecord(e1);
      if (hipEventSynchronize(e1) != hipSuccess) {
        fprintf(stderr, "launch %d failed\n", m);
        return 1;
      }
      float ms;
      (void)hipEventElapsedTime(&ms, e0, e1);
      if (rep > 0 && ms < best) best = ms;
    }
    const double seqs = double(blocks) * threads / 64 * iters * 64;  // sequences (or wave-instructions) per launch
    const double cyc = simds * hz / (seqs / (best * 1e-3));
    if (m == 0) fma_cyc = cyc;
    printf("{\"form\": \"%s\", \"ms\": %.3f, \"cycles_per_sequence_per_simd\": %.2f, \"vs_fma\": %.2f, \"clock_MHz\": %.0f}\n", names[m],
           best, cyc, cyc / fma_cyc, hz / 1e6);
  }
  return 0;
}
