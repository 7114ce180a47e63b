// tools/valubench4.hip — issue cost of the VALU forms behind the exact float
// sqrt (rtmi_path.h sqrt_cr) and sincos2pi's quadrant logic, against
// v_fma_f32 v,v,v,v: the transcendentals, compares writing VCC or an SGPR
// pair, the compare + select pattern of the neighbour form of sqrt_cr, the
// integer add, v_bitop3_b32; then whole sequences (the neighbour form
// sqrt_cr had before the v_rsq_f32 one, the 5- / 7- / 8-operation v_rsq_f32 +
// FMA forms, the two range guards), written in C++ as the header writes them
// and timed per sequence.  8 independent chains per
// lane, 8 waves per SIMD, as tools/valubench3.hip.  One JSON line per form:
// cycles per wave-instruction (or per sequence) per SIMD.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o valubench4 tools/valubench4.hip
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

enum Form {
  FMA, SQRT, RSQ, RCP, CMP_VCC, CMP_SGPR, CMP_CND, ADD_U32, BITOP3, NINSTR,
  SEQ_NEIGHBOUR = NINSTR, SEQ_RSQ5, SEQ_RSQ7, SEQ_RSQ8, SEQ_RSQ8_FLOAT_GUARD, SEQ_RSQ8_NO_GUARD, GUARD_UINT, GUARD_FLOAT,
  NFORMS
};

// ---- the sequences, as rtmi_path.h writes them --------------------------------
__device__ __forceinline__ float seq_neighbour(float x) {
  const bool slow = !(x >= 0x1p-96f);
  const float s = __builtin_amdgcn_sqrtf(x);
  const float sm = __int_as_float(__float_as_int(s) - 1), sp = __int_as_float(__float_as_int(s) + 1);
  float r = __builtin_fmaf(-sm, s, x) <= 0.0f ? sm : s;
  r = __builtin_fmaf(-sp, s, x) > 0.0f ? sp : r;
  if (__builtin_expect(__ballot(slow) != 0, 0)) {
    if (slow) r = __builtin_sqrtf(x);
  }
  return r;
}
template <int OPS> __device__ __forceinline__ float rsq_core(float x) {
  const float y = __builtin_amdgcn_rsqf(x);
  float g = x * y, h = 0.5f * y;
  if constexpr (OPS >= 7) {
    const float e = __builtin_fmaf(-h, g, 0.5f);
    g = __builtin_fmaf(g, e, g);
    if constexpr (OPS >= 8) h = __builtin_fmaf(h, e, h);
  }
  return __builtin_fmaf(__builtin_fmaf(-g, g, x), h, g);
}
__device__ __forceinline__ bool guard_uint(float x) { return __float_as_uint(x) - 0x0F800000u >= 0x70000000u; }
__device__ __forceinline__ bool guard_float(float x) { return !(x >= 0x1p-96f && x < __builtin_inff()); }
// GUARD 0: none, 1: one unsigned range test on the bits, 2: two float compares
template <int OPS, int GUARD> __device__ __forceinline__ float seq_rsq(float x) {
  float r = rsq_core<OPS>(x);
  if constexpr (GUARD != 0) {
    const bool slow = GUARD == 1 ? guard_uint(x) : guard_float(x);
    if (__builtin_expect(__ballot(slow) != 0, 0)) {
      if (slow) r = __builtin_sqrtf(x);
    }
  }
  return r;
}
// the guard alone on top of one v_add_f32 (subtract the ADD-only cost: v_add_f32 is 2.1 in valubench3's table)
template <int GUARD> __device__ __forceinline__ float seq_guard(float x) {
  float r = x + 0x1p-20f;
  const bool slow = GUARD == 1 ? guard_uint(x) : guard_float(x);
  if (__builtin_expect(__ballot(slow) != 0, 0)) {
    if (slow) r = __builtin_sqrtf(x);
  }
  return r;
}

template <int MODE>
__global__ __launch_bounds__(256) void k(float *out, int iters, unsigned long long mask) {
  float x0 = threadIdx.x + 1, x1 = x0 + 1, x2 = x0 + 2, x3 = x0 + 3, x4 = x0 + 4, x5 = x0 + 5, x6 = x0 + 6, x7 = x0 + 7;
  float va = 1.0000001f + threadIdx.x * 1e-12f, vb = 1e-7f;
  uint32_t ua = 2654435761u + threadIdx.x, ub = 40503u + threadIdx.x;
  unsigned long long m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0, m5 = 0, m6 = 0, m7 = 0;
#define ALL8(M) M(x0) M(x1) M(x2) M(x3) M(x4) M(x5) M(x6) M(x7)
#define ALL8M(M) M(m0, x0) M(m1, x1) M(m2, x2) M(m3, x3) M(m4, x4) M(m5, x5) M(m6, x6) M(m7, x7)
  for (int i = 0; i < iters; i++) {
#pragma unroll
    for (int r = 0; r < 8; r++) {
      if constexpr (MODE == FMA) {
#define F_FMA(x) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(x) : "v"(vb), "v"(va));
        ALL8(F_FMA)
      } else if constexpr (MODE == SQRT) {
#define F_SQRT(x) asm volatile("v_sqrt_f32 %0, %0" : "+v"(x));
        ALL8(F_SQRT)
      } else if constexpr (MODE == RSQ) {
#define F_RSQ(x) asm volatile("v_rsq_f32 %0, %0" : "+v"(x));
        ALL8(F_RSQ)
      } else if constexpr (MODE == RCP) {
#define F_RCP(x) asm volatile("v_rcp_f32 %0, %0" : "+v"(x));
        ALL8(F_RCP)
      } else if constexpr (MODE == CMP_VCC) {
        // (a compare writes no VGPR: the eight differ in their source)
#define F_CVCC(x) asm volatile("v_cmp_lt_f32 vcc, %0, %1" : : "v"(x), "v"(va) : "vcc");
        ALL8(F_CVCC)
      } else if constexpr (MODE == CMP_SGPR) {
#define F_CSG(m, x) asm volatile("v_cmp_lt_f32 %0, %1, %2" : "=s"(m) : "v"(x), "v"(va));
        ALL8M(F_CSG)
      } else if constexpr (MODE == CMP_CND) {
        // compare into an SGPR pair, the two wait states the hazard asks for, the select on it: two VALU
        // instructions (the table gives the cost of the pair)
#define F_CC(m, x) \
  asm volatile("v_cmp_lt_f32 %1, %0, %2\n\ts_nop 1\n\tv_cndmask_b32 %0, %0, %3, %1" : "+v"(x), "=&s"(m) : "v"(va), "v"(vb));
        ALL8M(F_CC)
      } else if constexpr (MODE == ADD_U32) {
#define F_ADDU(x) asm volatile("v_add_u32 %0, %1, %0" : "+v"(x) : "v"(ua));
        ALL8(F_ADDU)
      } else if constexpr (MODE == BITOP3) {
        // a ^ (b & c)
#define F_BO3(x) asm volatile("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x78" : "+v"(x) : "v"(ua), "v"(ub));
        ALL8(F_BO3)
      } else if constexpr (MODE == SEQ_NEIGHBOUR) {
#define F_SN(x) x = seq_neighbour(x);
        ALL8(F_SN)
      } else if constexpr (MODE == SEQ_RSQ5) {
#define F_S5(x) x = seq_rsq<5, 1>(x);
        ALL8(F_S5)
      } else if constexpr (MODE == SEQ_RSQ7) {
#define F_S7(x) x = seq_rsq<7, 1>(x);
        ALL8(F_S7)
      } else if constexpr (MODE == SEQ_RSQ8) {
#define F_S8(x) x = seq_rsq<8, 1>(x);
        ALL8(F_S8)
      } else if constexpr (MODE == SEQ_RSQ8_FLOAT_GUARD) {
#define F_S8F(x) x = seq_rsq<8, 2>(x);
        ALL8(F_S8F)
      } else if constexpr (MODE == SEQ_RSQ8_NO_GUARD) {
#define F_S8N(x) x = seq_rsq<8, 0>(x);
        ALL8(F_S8N)
      } else if constexpr (MODE == GUARD_UINT) {
#define F_GU(x) x = seq_guard<1>(x);
        ALL8(F_GU)
      } else {
#define F_GF(x) x = seq_guard<2>(x);
        ALL8(F_GF)
      }
    }
  }
  float s = x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7;
  s += float(m0 + m1 + m2 + m3 + m4 + m5 + m6 + m7);
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
  const char *names[NFORMS] = {"v_fma_f32 v,v,v,v", "v_sqrt_f32", "v_rsq_f32", "v_rcp_f32", "v_cmp_lt_f32 vcc",
                               "v_cmp_lt_f32 sgpr-pair", "v_cmp + s_nop 1 + v_cndmask_b32 (pair)", "v_add_u32",
                               "v_bitop3_b32", "seq: v_sqrt_f32 + neighbours", "seq: rsq 5-op, uint guard",
                               "seq: rsq 7-op, uint guard", "seq: rsq 8-op, uint guard", "seq: rsq 8-op, float guard",
                               "seq: rsq 8-op, no guard", "seq: v_add_f32 + uint guard", "seq: v_add_f32 + float guard"};
  void (*kern[NFORMS])(float *, int, unsigned long long) = {k<0>, k<1>, k<2>,  k<3>,  k<4>,  k<5>,  k<6>,  k<7>, k<8>,
                                                             k<9>, k<10>, k<11>, k<12>, k<13>, k<14>, k<15>, k<16>};
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
      hipLaunchKernelGGL(kern[m], dim3(blocks), dim3(threads), 0, 0, out, iters, 0x5555555555555555ull);
      (void)hipEventRecord(e1);
      if (hipEventSynchronize(e1) != hipSuccess) {
        fprintf(stderr, "launch %d failed\n", m);
        return 1;
      }
      float ms;
      (void)hipEventElapsedTime(&ms, e0, e1);
      if (rep > 0 && ms < best) best = ms;
    }
    const double instr = double(blocks) * threads / 64 * iters * 64;  // wave-instructions (or sequences)
    const double cyc = simds * hz / (instr / (best * 1e-3));
    if (m == 0) fma_cyc = cyc;
    printf("{\"form\": \"%s\", \"ms\": %.3f, \"cycles_per_wave_instr_per_simd\": %.2f, \"vs_fma\": %.2f, \"clock_MHz\": %.0f}\n",
           names[m], best, cyc, cyc / fma_cyc, hz / 1e6);
  }
  return 0;
}
