// tools/valubench6.hip — cost of the range guards of the exact float sqrt and
// reciprocal (rtmi_path.h sqrt_cr, rcp_cr) as whole dependent sequences, guards
// included, in C++ as the header writes them: 1 / sqrt(x) as rcp_cr(sqrt_cr(x))
// with its two guards against rsqrt_cr with one; rcp_cr's guard by two float
// compares against one unsigned test of the shifted bit pattern; sqrt_cr
// against the guard-free form for {+0} U [2^-96, inf); and sqrt_cr's short
// form guarded by a NaN test of its result (DESIGN §8 item 4's probe).  Every
// chain feeds its result back (x = f(x), which stays near 1).  8 independent
// chains per lane, 8 waves per SIMD, as tools/valubench4.hip.  One JSON line
// per form: cycles per sequence per SIMD.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o tools/valubench6_bin tools/valubench6.hip
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

enum Form { FMA, RSQRT_TWO_GUARDS, RSQRT_ONE_GUARD, RCP_FLOAT, RCP_UINT, SQRT_GUARDED, SQRT_ZERO_OR_BIG, SQRT_NAN_GUARD, NFORMS };

__device__ __forceinline__ float sqrt_short(float x) {
  const float y = __builtin_amdgcn_rsqf(x);
  const float g = x * y, h = 0.5f * y;
  return __builtin_fmaf(__builtin_fmaf(-g, g, x), h, g);
}
__device__ __forceinline__ float rcp_short(float x) {
  const float r0 = __builtin_amdgcn_rcpf(x);
  return __builtin_fmaf(__builtin_fmaf(-x, r0, 1.0f), r0, r0);
}
__device__ __forceinline__ bool sqrt_slow(float x) { return __float_as_uint(x) - 0x0F800000u >= 0x7F800000u - 0x0F800000u; }
__device__ __forceinline__ float sqrt_cr(float x) {
  const bool slow = sqrt_slow(x);
  float r = sqrt_short(x);
  if (__builtin_expect(__ballot(slow) != 0, 0)) {
    if (slow) r = __builtin_sqrtf(x);
  }
  return r;
}
template <bool UINT> __device__ __forceinline__ float rcp_cr(float x) {
  bool slow;
  if constexpr (UINT) slow = (__float_as_uint(x) << 1) - 0x02000000u > 0xFC000000u - 0x02000000u;
  else {
    const float ax = __builtin_fabsf(x);
    slow = !(ax >= 0x1p-125f && ax <= 0x1p+125f);
  }
  float r = rcp_short(x);
  if (__builtin_expect(__ballot(slow) != 0, 0)) {
    if (slow) r = 1.0f / x;
  }
  return r;
}
__device__ __forceinline__ float rsqrt_cr(float x) {
  const bool slow = sqrt_slow(x);
  float r = rcp_short(sqrt_short(x));
  if (__builtin_expect(__ballot(slow) != 0, 0)) {
    if (slow) r = 1.0f / __builtin_sqrtf(x);
  }
  return r;
}
__device__ __forceinline__ float sqrt_zero_or_big(float x) {
  const float y = __builtin_amdgcn_rsqf(__builtin_fmaxf(x, 0x1p-96f));
  const float g = x * y, h = 0.5f * y;
  return __builtin_fmaf(__builtin_fmaf(-g, g, x), h, g);
}
// the guard as a test of the result: every input outside [2^-96, inf) but the small normals ends in NaN
__device__ __forceinline__ float sqrt_nan_guard(float x) {
  float r = sqrt_short(x);
  const bool slow = r != r;
  if (__builtin_expect(__ballot(slow) != 0, 0)) {
    if (slow) r = __builtin_sqrtf(x);
  }
  return r;
}

template <int MODE>
__global__ __launch_bounds__(256) void k(float *out, int iters, float scale) {
  float x0 = (threadIdx.x + 1) * scale, x1 = x0 + 1, x2 = x0 + 2, x3 = x0 + 3, x4 = x0 + 4, x5 = x0 + 5, x6 = x0 + 6, x7 = x0 + 7;
  const float va = 1.0000001f + threadIdx.x * 1e-12f, vb = 1e-7f;
#define ALL8(M) M(x0) M(x1) M(x2) M(x3) M(x4) M(x5) M(x6) M(x7)
  for (int i = 0; i < iters; i++) {
#pragma unroll
    for (int r = 0; r < 8; r++) {
      if constexpr (MODE == FMA) {
#define F_FMA(x) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(x) : "v"(vb), "v"(va));
        ALL8(F_FMA)
      } else if constexpr (MODE == RSQRT_TWO_GUARDS) {
#define F_R2(x) x = rcp_cr<false>(sqrt_cr(x));
        ALL8(F_R2)
      } else if constexpr (MODE == RSQRT_ONE_GUARD) {
#define F_R1(x) x = rsqrt_cr(x);
        ALL8(F_R1)
      } else if constexpr (MODE == RCP_FLOAT) {
#define F_CF(x) x = rcp_cr<false>(x);
        ALL8(F_CF)
      } else if constexpr (MODE == RCP_UINT) {
#define F_CU(x) x = rcp_cr<true>(x);
        ALL8(F_CU)
      } else if constexpr (MODE == SQRT_GUARDED) {
#define F_SG(x) x = sqrt_cr(x);
        ALL8(F_SG)
      } else if constexpr (MODE == SQRT_ZERO_OR_BIG) {
#define F_SZ(x) x = sqrt_zero_or_big(x);
        ALL8(F_SZ)
      } else {
#define F_SN(x) x = sqrt_nan_guard(x);
        ALL8(F_SN)
      }
    }
  }
  const float s = x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7;
  if (s == 12345.f) out[0] = s;
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
                               "1/sqrt: rcp_cr(sqrt_cr(x)), two guards (parent)",
                               "1/sqrt: rsqrt_cr, one guard",
                               "rcp_cr: two float compares (parent)",
                               "rcp_cr: one unsigned range test",
                               "sqrt_cr: unsigned guard (parent)",
                               "sqrt for {+0} U [2^-96, inf): max, no guard",
                               "sqrt: guard on the result (r != r)"};
  void (*kern[NFORMS])(float *, int, float) = {k<0>, k<1>, k<2>, k<3>, k<4>, k<5>, k<6>, k<7>};
  int clock_khz = 0;
  (void)hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeClockRate, 0);
  const double hz = clock_khz > 0 ? clock_khz * 1e3 : 2.4e9;
  int cus = 0;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
  const double simds = 4.0 * (cus > 0 ? cus : 256);
  double fma_cyc = 0;
  for (int pass = 0; pass < 2; pass++) {  // the second pass shows the repeatability
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
      printf("{\"pass\": %d, \"form\": \"%s\", \"ms\": %.3f, \"cycles_per_sequence_per_simd\": %.2f, \"vs_fma\": %.2f, \"clock_MHz\": %.0f}\n",
             pass, names[m], best, cyc, cyc / fma_cyc, hz / 1e6);
    }
  }
  return 0;
}
