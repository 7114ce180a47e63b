// rtmi_nw_denoise.hip — the Next-Week renderer's denoiser: an edge-avoiding a-trous wavelet filter guided by
// first-hit features and the per-pixel variance (include/rtmi_nw.h "Denoising"; DESIGN.md §9 "Denoising").
//
// Three kernels, 16 x 16 pixels per 256-thread block, one pixel per lane (a wave covers 16 x 4 pixels, so a row of
// a wave's load is 16 float4 = one contiguous 256-byte segment):
//   prepare   colour / albedo and variance / albedo^2 into P0 = {c'.rgb, v'}, the guides into P1 = {n.xyz, z},
//             the depth slope gz beside them;
//   pass      one 5 x 5 B3 level at a power-of-two step, P0 -> P0 (two images used in turn); every tap is one
//             float4 load of P0 and one of P1, straight from global memory (the images of a frame live in L2 and
//             the Infinity Cache), and one exponential (v_exp_f32);
//   finish    c' * albedo, v' * albedo^2.
// The header's formulas are the specification; tests/nw_denoise_model.py restates them in float64.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rtmi_internal.h"
#include "rtmi_nw_internal.h"

namespace rtmi {
namespace nw {

constexpr int kDnTile = 16;
constexpr float kAlbedoFloor = 0.01f;

struct DnImage {
  int32_t W, H;
};

struct DnPass {
  int32_t W, H, step;
  float half_sigma_n, sigma_z, sigma_l;
  int32_t edges, lum;  // edges: the edge weights are on; lum: there is a variance guide
};

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool finite3(const float4 &c) { return finite_f(c.x) && finite_f(c.y) && finite_f(c.z); }

// the demodulation albedo of a pixel: {A.rgb, Abar}
__device__ __forceinline__ float4 albedo_of(const float *__restrict__ f, int demod) {
  if (!demod) return make_float4(1.0f, 1.0f, 1.0f, 1.0f);
  const float r = fmaxf(f[0], kAlbedoFloor), g = fmaxf(f[1], kAlbedoFloor), b = fmaxf(f[2], kAlbedoFloor);
  return make_float4(r, g, b, ((r + g) + b) / 3.0f);
}

// the difference of z along one axis: over the in-image neighbours with cov > 0 (lo, hi: their pixel indices or -1)
__device__ __forceinline__ float z_slope(const float *__restrict__ feat, float zp, long lo, long hi) {
  const bool has_lo = lo >= 0 && feat[8 * lo + 7] > 0.0f, has_hi = hi >= 0 && feat[8 * hi + 7] > 0.0f;
  if (has_lo && has_hi) return (feat[8 * hi + 6] - feat[8 * lo + 6]) * 0.5f;
  if (has_hi) return feat[8 * hi + 6] - zp;
  if (has_lo) return zp - feat[8 * lo + 6];
  return 0.0f;
}

__global__ __launch_bounds__(256) void dn_prepare_kernel(const float *__restrict__ color, const float *__restrict__ var,
                                                         const float *__restrict__ feat, float4 *__restrict__ p0,
                                                         float4 *__restrict__ p1, float *__restrict__ gz, DnImage im, int demod) {
  const int x = blockIdx.x * kDnTile + (threadIdx.x & 15), y = blockIdx.y * kDnTile + (threadIdx.x >> 4);
  if (x >= im.W || y >= im.H) return;
  const long p = long(y) * im.W + x;
  const float *f = feat + 8 * p;
  const float4 a = albedo_of(f, demod);
  const float v = var ? var[p] / (a.w * a.w) : 0.0f;
  p0[p] = make_float4(color[3 * p] / a.x, color[3 * p + 1] / a.y, color[3 * p + 2] / a.z, v);
  const float z = f[6];
  p1[p] = make_float4(f[3], f[4], f[5], z);
  const float gx = z_slope(feat, z, x > 0 ? p - 1 : -1, x + 1 < im.W ? p + 1 : -1);
  const float gy = z_slope(feat, z, y > 0 ? p - im.W : -1, y + 1 < im.H ? p + im.W : -1);
  gz[p] = fmaxf(fabsf(gx), fabsf(gy));
}

__global__ __launch_bounds__(256) void dn_pass_kernel(const float4 *__restrict__ in, const float4 *__restrict__ p1,
                                                      const float *__restrict__ gz, float4 *__restrict__ out, DnPass a) {
  const int x = blockIdx.x * kDnTile + (threadIdx.x & 15), y = blockIdx.y * kDnTile + (threadIdx.x >> 4);
  if (x >= a.W || y >= a.H) return;
  const long p = long(y) * a.W + x;
  const float4 cp = in[p];
  if (!finite3(cp)) {  // passes through unchanged
    out[p] = cp;
    return;
  }
  const float4 gp = p1[p];
  const bool var_ok = finite_f(cp.w);
  const bool lum = a.edges && a.lum && var_ok;
  float inv_sd = 0.0f;
  if (lum) {  // the 3 x 3 binomial mean of v' around p, over the in-image pixels whose v' is finite
    float sv = 0.0f, sk = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = y + dy;
      if (yy < 0 || yy >= a.H) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        const int xx = x + dx;
        if (xx < 0 || xx >= a.W) continue;
        const float v = in[long(yy) * a.W + xx].w;
        if (!finite_f(v)) continue;
        const float k = (dx ? 0.25f : 0.5f) * (dy ? 0.25f : 0.5f);
        sv = __builtin_fmaf(k, v, sv);
        sk += k;
      }
    }
    inv_sd = 1.0f / __builtin_fmaf(a.sigma_l, sqrtf(fmaxf(sv / sk, 0.0f)), 1e-6f);
  }
  const float lp = (cp.x + cp.y) + cp.z;
  const float z_slope_scale = a.sigma_z * gz[p] * float(a.step), z_base = __builtin_fmaf(1e-3f, fabsf(gp.w), 1e-12f);
  const float wc = 9.0f / 64.0f;
  float sw = wc, sr = wc * cp.x, sg = wc * cp.y, sb = wc * cp.z, s2 = var_ok ? (wc * wc) * cp.w : 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int yy = y + dy * a.step;
    if (yy < 0 || yy >= a.H) continue;
    const float hy = dy == 0 ? 0.375f : (dy == 1 || dy == -1) ? 0.25f : 0.0625f;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      if (dx == 0 && dy == 0) continue;
      const int xx = x + dx * a.step;
      if (xx < 0 || xx >= a.W) continue;
      const long q = long(yy) * a.W + xx;
      const float4 cq = in[q];
      if (!finite3(cq) || !finite_f(cq.w)) continue;
      const float hx = dx == 0 ? 0.375f : (dx == 1 || dx == -1) ? 0.25f : 0.0625f;
      float w = hx * hy;
      if (a.edges) {
        const float4 gq = p1[q];
        const float nx = gp.x - gq.x, ny = gp.y - gq.y, nz = gp.z - gq.z;
        const float dn2 = __builtin_fmaf(nz, nz, __builtin_fmaf(ny, ny, nx * nx));
        const int r = (dx < 0 ? -dx : dx) > (dy < 0 ? -dy : dy) ? (dx < 0 ? -dx : dx) : (dy < 0 ? -dy : dy);
        float arg = __builtin_fmaf(a.half_sigma_n, dn2, fabsf(gp.w - gq.w) / __builtin_fmaf(z_slope_scale, float(r), z_base));
        if (lum) arg = __builtin_fmaf(fabsf(lp - ((cq.x + cq.y) + cq.z)), inv_sd, arg);
        w *= __builtin_amdgcn_exp2f(arg * -1.44269504f);  // exp(-arg): one v_exp_f32
        if (!finite_f(w)) continue;
      }
      sw += w;
      sr = __builtin_fmaf(w, cq.x, sr);
      sg = __builtin_fmaf(w, cq.y, sg);
      sb = __builtin_fmaf(w, cq.z, sb);
      s2 = __builtin_fmaf(w * w, cq.w, s2);
    }
  }
  out[p] = make_float4(sr / sw, sg / sw, sb / sw, var_ok ? s2 / (sw * sw) : cp.w);
}

__global__ __launch_bounds__(256) void dn_finish_kernel(const float4 *__restrict__ p0, const float *__restrict__ feat,
                                                        float *__restrict__ out, float *__restrict__ var_out, DnImage im, int demod) {
  const int x = blockIdx.x * kDnTile + (threadIdx.x & 15), y = blockIdx.y * kDnTile + (threadIdx.x >> 4);
  if (x >= im.W || y >= im.H) return;
  const long p = long(y) * im.W + x;
  const float4 a = albedo_of(feat + 8 * p, demod);
  const float4 c = p0[p];
  out[3 * p] = c.x * a.x;
  out[3 * p + 1] = c.y * a.y;
  out[3 * p + 2] = c.z * a.z;
  if (var_out) var_out[p] = c.w * (a.w * a.w);
}

}  // namespace nw
}  // namespace rtmi

using namespace rtmi;
using namespace rtmi::nw;

namespace {

constexpr size_t kDnBytesPerPixel = 3 * sizeof(float4) + sizeof(float);

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

struct TurnEnd {
  rt_nw_ctx *c;
  void *s;
  ~TurnEnd() { ctx_end(c, s); }
};

int check_denoise_args(const char *who, rt_nw_ctx *ctx, int32_t W, int32_t H, const float *color, const float *feat,
                       const rt_nw_denoise_params *p, const float *out, rt_nw_denoise_params &use) {
  if (!ctx || !color || !feat || !out) return set_error(RT_EINVAL, "%s: null argument", who);
  if (W < 1 || H < 1 || int64_t(W) * H >= (int64_t(1) << 31)) return set_error(RT_EINVAL, "%s: bad size %dx%d", who, W, H);
  if (p) use = *p;
  else if (int rc = rt_nw_denoise_params_default(&use)) return rc;
  return rt_nw_denoise_params_check(&use);
}

}  // namespace

RTMI_EXPORT int rt_nw_denoise(rt_nw_ctx *ctx, int32_t W, int32_t H, const float *dev_color, const float *dev_var,
                              const float *dev_feat, const rt_nw_denoise_params *p, float *dev_out, float *dev_var_out,
                              void *stream) {
  rt_nw_denoise_params use;
  if (int rc = check_denoise_args("rt_nw_denoise", ctx, W, H, dev_color, dev_feat, p, dev_out, use)) return rc;
  CtxLink link;
  if (int rc = ctx_link(ctx, link)) return rc;
  DeviceGuard g(link.device);
  const size_t npix = size_t(W) * size_t(H);
  if (link.scratch->pixels < npix) {  // (nothing of the context may still read the old images)
    if (int rc = ctx_idle(ctx)) return rc;
    if (link.scratch->p) (void)hipFree(link.scratch->p);
    link.scratch->p = nullptr;
    link.scratch->pixels = 0;
    const hipError_t e = hipMalloc(&link.scratch->p, npix * kDnBytesPerPixel);
    if (e != hipSuccess) {
      link.scratch->p = nullptr;
      return set_error(RT_ENOMEM, "rt_nw_denoise: hipMalloc(%zu B): %s", npix * kDnBytesPerPixel, hipGetErrorString(e));
    }
    link.scratch->pixels = npix;
  }
  // the images are laid out for the allocation's capacity, so a smaller frame uses their heads
  float4 *img[2] = {static_cast<float4 *>(link.scratch->p), static_cast<float4 *>(link.scratch->p) + link.scratch->pixels};
  float4 *p1 = img[1] + link.scratch->pixels;
  float *gz = reinterpret_cast<float *>(p1 + link.scratch->pixels);
  void *st_v = stream ? stream : link.stream;
  hipStream_t st = static_cast<hipStream_t>(st_v);
  if (int rc = ctx_begin(ctx, st_v)) return rc;
  TurnEnd end{ctx, st_v};
  const dim3 grid(unsigned((W + kDnTile - 1) / kDnTile), unsigned((H + kDnTile - 1) / kDnTile)), block(256);
  const int demod = (use.flags & RT_NW_DENOISE_DEMODULATE) ? 1 : 0;
  const DnImage im{W, H};
  hipLaunchKernelGGL(dn_prepare_kernel, grid, block, 0, st, dev_color, dev_var, dev_feat, img[0], p1, gz, im, demod);
  int cur = 0;
  for (int k = 0; k < use.iterations; ++k) {
    const DnPass a{W, H, 1 << k, 0.5f * use.sigma_n, use.sigma_z, use.sigma_l, (use.flags & RT_NW_DENOISE_NO_EDGES) ? 0 : 1,
                   dev_var ? 1 : 0};
    hipLaunchKernelGGL(dn_pass_kernel, grid, block, 0, st, img[cur], p1, gz, img[cur ^ 1], a);
    cur ^= 1;
  }
  hipLaunchKernelGGL(dn_finish_kernel, grid, block, 0, st, img[cur], dev_feat, dev_out, dev_var ? dev_var_out : nullptr, im, demod);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(RT_EHIP, "rt_nw_denoise: %s", hipGetErrorString(e));
  return RT_OK;
}

RTMI_EXPORT int rt_nw_denoise_host(rt_nw_ctx *ctx, int32_t W, int32_t H, const float *color, const float *var, const float *feat,
                                   const rt_nw_denoise_params *p, float *out, float *var_out) {
  rt_nw_denoise_params use;
  if (int rc = check_denoise_args("rt_nw_denoise_host", ctx, W, H, color, feat, p, out, use)) return rc;
  CtxLink link;
  if (int rc = ctx_link(ctx, link)) return rc;
  DeviceGuard g(link.device);
  const size_t npix = size_t(W) * size_t(H);
  // one allocation: color | feat | out | var | var_out
  float *d = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&d), npix * 16 * sizeof(float));
  if (e != hipSuccess) return set_error(RT_ENOMEM, "rt_nw_denoise_host: hipMalloc: %s", hipGetErrorString(e));
  float *d_color = d, *d_feat = d + 3 * npix, *d_out = d + 11 * npix, *d_var = d + 14 * npix, *d_vout = d + 15 * npix;
  hipStream_t st = static_cast<hipStream_t>(link.stream);
  e = hipMemcpyAsync(d_color, color, npix * 3 * sizeof(float), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_feat, feat, npix * 8 * sizeof(float), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && var) e = hipMemcpyAsync(d_var, var, npix * sizeof(float), hipMemcpyHostToDevice, st);
  int rc = RT_OK;
  if (e == hipSuccess) rc = rt_nw_denoise(ctx, W, H, d_color, var ? d_var : nullptr, d_feat, &use, d_out, var_out ? d_vout : nullptr, nullptr);
  if (rc == RT_OK && e == hipSuccess) e = hipMemcpyAsync(out, d_out, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, st);
  if (rc == RT_OK && e == hipSuccess && var && var_out) e = hipMemcpyAsync(var_out, d_vout, npix * sizeof(float), hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);
  (void)hipFree(d);
  if (rc != RT_OK) return rc;
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return set_error(RT_EHIP, "rt_nw_denoise_host: %s", hipGetErrorString(e));
  return RT_OK;
}
