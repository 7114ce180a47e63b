// tools/valubench3.hip — issue cost of the VALU forms the grid kernel's
// per-segment prologue uses or could use (ray terms, big spheres, box clip,
// DDA setup, job decode), against v_fma_f32 v,v,v,v.  Inline asm, 8
// independent chains per lane, 8 waves per SIMD, as tools/valubench2.hip.
// Prints one JSON line per form: cycles per wave-instruction per SIMD.
//   hipcc --offload-arch=gfx950 -O2 -o valubench3 tools/valubench3.hip
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

typedef float f2 __attribute__((ext_vector_type(2)));

enum Form {
  FMA, MUL_LO, MUL_HI, MAD_U64, MUL_U24, MAD_U24, CVT_F32_I32, CVT_I32_F32, FLOOR, MED3_I32, MED3_F32, CND_VCC,
  CND_SGPR, PK_DUP, PK_BCAST, PK_BCAST_HI, MOV, LSHR, AND, ADD_F32, MAX_F32, BFI, CND_VCC_VCMP, NFORMS
};

template <int MODE>
__global__ __launch_bounds__(256) void k(float *out, int iters, unsigned long long mask) {
  float x0 = threadIdx.x, x1 = x0 + 1, x2 = x0 + 2, x3 = x0 + 3, x4 = x0 + 4, x5 = x0 + 5, x6 = x0 + 6, x7 = x0 + 7;
  float va = 1.0000001f + threadIdx.x * 1e-12f, vb = 1e-7f;
  uint32_t ua = 2654435761u + threadIdx.x, ub = 40503u + threadIdx.x;
  uint64_t w0 = threadIdx.x, w1 = w0 + 1, w2 = w0 + 2, w3 = w0 + 3, w4 = w0 + 4, w5 = w0 + 5, w6 = w0 + 6, w7 = w0 + 7;
  f2 p0 = {x0, x1}, p1 = {x2, x3}, p2 = {x4, x5}, p3 = {x6, x7}, p4 = p0 + 8.f, p5 = p1 + 8.f, p6 = p2 + 8.f, p7 = p3 + 8.f;
  f2 pa = {va, va}, pb = {vb, vb};
  f2 pab = {va, vb};  // one pair, its halves broadcast by op_sel / op_sel_hi
#define ALL8(M) M(x0) M(x1) M(x2) M(x3) M(x4) M(x5) M(x6) M(x7)
#define ALL8W(M) M(w0) M(w1) M(w2) M(w3) M(w4) M(w5) M(w6) M(w7)
#define ALL8P(M) M(p0) M(p1) M(p2) M(p3) M(p4) M(p5) M(p6) M(p7)
  for (int i = 0; i < iters; i++) {
    // the mask in VCC: moved there by the scalar unit, or written by a vector compare
    if constexpr (MODE == CND_VCC) asm volatile("s_mov_b64 vcc, %0" : : "s"(mask) : "vcc");
    if constexpr (MODE == CND_VCC_VCMP) asm volatile("v_cmp_lt_f32 vcc, %0, %1" : : "v"(vb), "v"(va) : "vcc");
#pragma unroll
    for (int r = 0; r < 8; r++) {
      if constexpr (MODE == FMA) {
#define F_FMA(x) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(x) : "v"(vb), "v"(va));
        ALL8(F_FMA)
      } else if constexpr (MODE == MUL_LO) {
#define F_MLO(x) asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(x) : "v"(ua));
        ALL8(F_MLO)
      } else if constexpr (MODE == MUL_HI) {
#define F_MHI(x) asm volatile("v_mul_hi_u32 %0, %0, %1" : "+v"(x) : "v"(ua));
        ALL8(F_MHI)
      } else if constexpr (MODE == MAD_U64) {
#define F_M64(w) asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(w) : "v"(ua), "v"(ub) : "vcc");
        ALL8W(F_M64)
      } else if constexpr (MODE == MUL_U24) {
#define F_M24(x) asm volatile("v_mul_u32_u24 %0, %0, %1" : "+v"(x) : "v"(ua));
        ALL8(F_M24)
      } else if constexpr (MODE == MAD_U24) {
#define F_MA24(x) asm volatile("v_mad_u32_u24 %0, %1, %2, %0" : "+v"(x) : "v"(ua), "v"(ub));
        ALL8(F_MA24)
      } else if constexpr (MODE == CVT_F32_I32) {
#define F_CFI(x) asm volatile("v_cvt_f32_i32 %0, %0" : "+v"(x));
        ALL8(F_CFI)
      } else if constexpr (MODE == CVT_I32_F32) {
#define F_CIF(x) asm volatile("v_cvt_i32_f32 %0, %0" : "+v"(x));
        ALL8(F_CIF)
      } else if constexpr (MODE == FLOOR) {
#define F_FLR(x) asm volatile("v_floor_f32 %0, %0" : "+v"(x));
        ALL8(F_FLR)
      } else if constexpr (MODE == MED3_I32) {
#define F_M3I(x) asm volatile("v_med3_i32 %0, %0, %1, %2" : "+v"(x) : "v"(ua), "v"(ub));
        ALL8(F_M3I)
      } else if constexpr (MODE == MED3_F32) {
#define F_M3F(x) asm volatile("v_med3_f32 %0, %0, %1, %2" : "+v"(x) : "v"(vb), "v"(va));
        ALL8(F_M3F)
      } else if constexpr (MODE == CND_VCC || MODE == CND_VCC_VCMP) {
#define F_CV(x) asm volatile("v_cndmask_b32 %0, %0, %1, vcc" : "+v"(x) : "v"(va));
        ALL8(F_CV)
      } else if constexpr (MODE == CND_SGPR) {
#define F_CS(x) asm volatile("v_cndmask_b32 %0, %0, %1, %2" : "+v"(x) : "v"(va), "s"(mask));
        ALL8(F_CS)
      } else if constexpr (MODE == PK_DUP) {
#define F_PD(p) asm volatile("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(p) : "v"(pb), "v"(pa));
        ALL8P(F_PD)
      } else if constexpr (MODE == PK_BCAST) {
        // both halves of source 0 read the pair's low register
#define F_PB(p) asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(p) : "v"(pab), "v"(pa));
        ALL8P(F_PB)
      } else if constexpr (MODE == PK_BCAST_HI) {
        // both halves of source 0 read the pair's high register
#define F_PH(p) asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(p) : "v"(pab), "v"(pa));
        ALL8P(F_PH)
      } else if constexpr (MODE == LSHR) {
#define F_SHR(x) asm volatile("v_lshrrev_b32 %0, 3, %0" : "+v"(x));
        ALL8(F_SHR)
      } else if constexpr (MODE == AND) {
#define F_AND(x) asm volatile("v_and_b32 %0, %1, %0" : "+v"(x) : "v"(ua));
        ALL8(F_AND)
      } else if constexpr (MODE == ADD_F32) {
#define F_ADD(x) asm volatile("v_add_f32 %0, %1, %0" : "+v"(x) : "v"(vb));
        ALL8(F_ADD)
      } else if constexpr (MODE == MAX_F32) {
#define F_MAX(x) asm volatile("v_max_f32 %0, %1, %0" : "+v"(x) : "v"(vb));
        ALL8(F_MAX)
      } else if constexpr (MODE == BFI) {
#define F_BFI(x) asm volatile("v_bfi_b32 %0, %1, %2, %0" : "+v"(x) : "v"(ua), "v"(ub));
        ALL8(F_BFI)
      } else {
#define F_MOV(x) asm volatile("v_mov_b32 %0, %0" : "+v"(x));
        ALL8(F_MOV)
      }
    }
  }
  float s = x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7;
  s += float(w0 + w1 + w2 + w3 + w4 + w5 + w6 + w7);
  const f2 ps = p0 + p1 + p2 + p3 + p4 + p5 + p6 + p7;
  s += ps.x + ps.y;
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
  const char *names[NFORMS] = {"v_fma_f32 v,v,v,v", "v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u64_u32", "v_mul_u32_u24",
                               "v_mad_u32_u24", "v_cvt_f32_i32", "v_cvt_i32_f32", "v_floor_f32", "v_med3_i32",
                               "v_med3_f32", "v_cndmask_b32 vcc", "v_cndmask_b32 sgpr-pair", "v_pk_fma_f32 dup pair",
                               "v_pk_fma_f32 op_sel_hi lo bcast", "v_pk_fma_f32 op_sel hi bcast", "v_mov_b32",
                               "v_lshrrev_b32", "v_and_b32", "v_add_f32", "v_max_f32", "v_bfi_b32",
                               "v_cndmask_b32 vcc (from v_cmp)"};
  void (*kern[NFORMS])(float *, int, unsigned long long) = {k<0>, k<1>, k<2>,  k<3>,  k<4>,  k<5>,  k<6>,  k<7>, k<8>,
                                                             k<9>, k<10>, k<11>, k<12>, k<13>, k<14>, k<15>, k<16>,
                                                             k<17>, k<18>, k<19>, k<20>, k<21>, k<22>};
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
    const double instr = double(blocks) * threads / 64 * iters * 64;  // wave-instructions
    const double cyc = simds * hz / (instr / (best * 1e-3));
    if (m == 0) fma_cyc = cyc;
    printf("{\"form\": \"%s\", \"ms\": %.3f, \"cycles_per_wave_instr_per_simd\": %.2f, \"vs_fma\": %.2f, \"clock_MHz\": %.0f}\n",
           names[m], best, cyc, cyc / fma_cyc, hz / 1e6);
  }
  return 0;
}
