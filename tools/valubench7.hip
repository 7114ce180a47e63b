// tools/valubench7.hip — the big-sphere group (rtmi_path.h hit_big: one group
// of four spheres) as a whole dependent sequence in C++ as the header writes
// it, in two forms: the ray terms duplicated into register pairs and 16
// v_pk_fma_f32 on sphere pairs (the parent; and the same without the copies,
// the halves broadcast by op_sel_hi), against 32 v_fma_f32 on single
// spheres, each taking its sphere value as the one scalar operand the constant
// bus allows.  The sphere data are wave-uniform and reach both forms through
// the constant address space (scalar registers), and both end in the group's
// candidate mask, which feeds back into the ray term K, so a call depends on
// the one before it.  The ray terms are made opaque at every call, as a new
// segment's are: the packed form has to duplicate them again.  One chain per
// lane, 8 waves per SIMD.  One JSON line per form: cycles per call per SIMD.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize -o tools/valubench7_bin tools/valubench7.hip
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

typedef float f2v __attribute__((ext_vector_type(2)));
struct SpherePair {
  f2v cx, cy, cz, S;
};
struct Sphere {
  float cx, cy, cz, S;
};

enum Form { FMA, PACKED, PACKED_OPSEL, PLAIN, NFORMS };

__device__ __forceinline__ unsigned cand(float x, int bit) { return (__float_as_int(x) >= 0 ? 1u : 0u) << bit; }

__device__ __forceinline__ unsigned group_packed(const SpherePair *pairs, f2v DX, f2v DY, f2v DZ, f2v KK, f2v AA, f2v AL,
                                                 f2v MX, f2v MY, f2v MZ) {
  typedef const __attribute__((address_space(4))) SpherePair *cpair_t;
  const cpair_t cp = (cpair_t)(size_t)pairs;
  auto pair = [&](int q, f2v &hb, f2v &disc) {
    const f2v cx = cp[q].cx, cy = cp[q].cy, cz = cp[q].cz, S = cp[q].S;
    const f2v hz = __builtin_elementwise_fma(-cz, DZ, KK);
    hb = __builtin_elementwise_fma(-cx, DX, __builtin_elementwise_fma(-cy, DY, hz));
    const f2v ac = __builtin_elementwise_fma(MX, cx, __builtin_elementwise_fma(MY, cy,
                   __builtin_elementwise_fma(MZ, cz, __builtin_elementwise_fma(AA, S, AL))));
    disc = __builtin_elementwise_fma(hb, hb, -ac);
  };
  f2v hb0, d0, hb1, d1;
  pair(0, hb0, d0);
  pair(1, hb1, d1);
  return cand(d0.x, 0) | cand(d0.y, 1) | cand(d1.x, 2) | cand(d1.y, 3);
}

__device__ __forceinline__ unsigned group_plain(const Sphere *sph, float dx, float dy, float dz, float K, float a, float aL,
                                                float mx, float my, float mz) {
  typedef const __attribute__((address_space(4))) Sphere *csph_t;
  const csph_t cs = (csph_t)(size_t)sph;
  auto one = [&](int j) {
    const float cx = cs[j].cx, cy = cs[j].cy, cz = cs[j].cz, S = cs[j].S;
    const float hb = __builtin_fmaf(-cx, dx, __builtin_fmaf(-cy, dy, __builtin_fmaf(-cz, dz, K)));
    const float ac = __builtin_fmaf(mx, cx, __builtin_fmaf(my, cy, __builtin_fmaf(mz, cz, __builtin_fmaf(a, S, aL))));
    return __builtin_fmaf(hb, hb, -ac);
  };
  return cand(one(0), 0) | cand(one(1), 1) | cand(one(2), 2) | cand(one(3), 3);
}

template <int MODE>
__global__ __launch_bounds__(256) void k(float *out, const SpherePair *pairs, const Sphere *sph, int iters) {
  const float t = float(threadIdx.x);
  float dx = 0.5f + 1e-3f * t, dy = -0.3f, dz = 0.4f, K = 1.0f + t, a = 0.5f, aL = 30.0f, mx = -1.0f, my = -2.0f, mz = -3.0f;
  const float va = 1.0000001f + threadIdx.x * 1e-12f, vb = 1e-7f;
  for (int i = 0; i < iters; i++) {
    if constexpr (MODE == FMA) {
#pragma unroll
      for (int r = 0; r < 32; r++) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(K) : "v"(vb), "v"(va));
    } else {
      // a new segment's ray terms: nothing of the last call's pairs survives
      asm volatile("" : "+v"(dx), "+v"(dy), "+v"(dz), "+v"(a), "+v"(aL), "+v"(mx), "+v"(my), "+v"(mz));
      unsigned m;
      if constexpr (MODE == PLAIN) {
        m = group_plain(sph, dx, dy, dz, K, a, aL, mx, my, mz);
      } else {
        f2v DX = {dx, dx}, DY = {dy, dy}, DZ = {dz, dz}, KK = {K, K}, AA = {a, a}, AL = {aL, aL};
        f2v MX = {mx, mx}, MY = {my, my}, MZ = {mz, mz};
        // PACKED: the nine pairs in registers of their own, as the render
        // kernels hold them through hit_big's loop over the groups (nine
        // v_mov_b32 a call).  Without that the compiler broadcasts the low
        // halves with op_sel_hi and copies nothing, which it does for this
        // one group and does not do in the kernels.
        if constexpr (MODE == PACKED) {
          asm volatile("" : "+v"(DX), "+v"(DY), "+v"(DZ), "+v"(KK), "+v"(AA), "+v"(AL), "+v"(MX), "+v"(MY), "+v"(MZ));
          dx = DX.x, dy = DY.x, dz = DZ.x, K = KK.x, a = AA.x, aL = AL.x, mx = MX.x, my = MY.x, mz = MZ.x;
        }
        m = group_packed(pairs, DX, DY, DZ, KK, AA, AL, MX, MY, MZ);
      }
      K += float(m) * 0x1p-20f;  // (both forms pay this conversion and FMA)
    }
  }
  if (K == 12345.f) out[0] = K;
}

int main() {
  float *out;
  if (hipMalloc(&out, 4) != hipSuccess) {
    fprintf(stderr, "no device\n");
    return 1;
  }
  // the final scene's big group: the ground and the three r = 1 spheres, {c, S = |c|^2 - r^2}
  const Sphere h_sph[4] = {{0.f, -1000.f, 0.f, 0.f}, {0.f, 1.f, 0.f, 0.f}, {-4.f, 1.f, 0.f, 16.f}, {4.f, 1.f, 0.f, 16.f}};
  SpherePair h_pairs[2];
  for (int q = 0; q < 2; q++) {
    h_pairs[q].cx = f2v{h_sph[2 * q].cx, h_sph[2 * q + 1].cx};
    h_pairs[q].cy = f2v{h_sph[2 * q].cy, h_sph[2 * q + 1].cy};
    h_pairs[q].cz = f2v{h_sph[2 * q].cz, h_sph[2 * q + 1].cz};
    h_pairs[q].S = f2v{h_sph[2 * q].S, h_sph[2 * q + 1].S};
  }
  SpherePair *pairs;
  Sphere *sph;
  if (hipMalloc(&pairs, sizeof(h_pairs)) != hipSuccess || hipMalloc(&sph, sizeof(h_sph)) != hipSuccess ||
      hipMemcpy(pairs, h_pairs, sizeof(h_pairs), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(sph, h_sph, sizeof(h_sph), hipMemcpyHostToDevice) != hipSuccess) {
    fprintf(stderr, "no device memory\n");
    return 1;
  }
  // 256 CUs x 4 SIMDs x 8 waves, 4 rounds of them
  const int blocks = 256 * 8 * 4, threads = 256, iters = 4000;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  const char *names[NFORMS] = {"32 x v_fma_f32 v,v,v,v", "big group: 9 duplications + 16 v_pk_fma_f32 (parent)",
                               "big group: 16 v_pk_fma_f32, low halves broadcast by op_sel_hi",
                               "big group: 32 v_fma_f32, one scalar operand each"};
  void (*kern[NFORMS])(float *, const SpherePair *, const Sphere *, int) = {k<0>, k<1>, k<2>, k<3>};
  int clock_khz = 0;
  (void)hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeClockRate, 0);
  const double hz = clock_khz > 0 ? clock_khz * 1e3 : 2.4e9;
  int cus = 0;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
  const double simds = 4.0 * (cus > 0 ? cus : 256);
  for (int pass = 0; pass < 2; pass++) {  // the second pass shows the repeatability
    for (int m = 0; m < NFORMS; m++) {
      float best = 1e30f;
      for (int rep = 0; rep < 3; rep++) {
        (void)hipEventRecord(e0);
        hipLaunchKernelGGL(kern[m], dim3(blocks), dim3(threads), 0, 0, out, pairs, sph, iters);
        (void)hipEventRecord(e1);
        if (hipEventSynchronize(e1) != hipSuccess) {
          fprintf(stderr, "launch %d failed\n", m);
          return 1;
        }
        float ms;
        (void)hipEventElapsedTime(&ms, e0, e1);
        if (rep > 0 && ms < best) best = ms;
      }
      const double calls = double(blocks) * threads / 64 * iters;  // wave-level calls per launch
      const double cyc = simds * hz / (calls / (best * 1e-3));
      printf("{\"pass\": %d, \"form\": \"%s\", \"ms\": %.3f, \"cycles_per_call_per_simd\": %.2f, \"clock_MHz\": %.0f}\n", pass,
             names[m], best, cyc, hz / 1e6);
    }
  }
  return 0;
}
