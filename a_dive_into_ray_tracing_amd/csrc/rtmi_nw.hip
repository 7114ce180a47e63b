// rtmi_nw.hip — gfx950 kernel and device C ABI of the Next-Week renderer
// (include/rtmi_nw.h).
//
// Same execution design as the RTIOW kernel (rtmi_device.hip render_kernel):
// one wavefront owns a work item = (8x8 pixel tile, range of samples); lanes
// pull (pixel, sample) jobs from a wave-local queue and regenerate paths as
// theirs terminate (__ballot + mbcnt compaction); colours are summed as int64
// fixed point in LDS, then one global atomic per pixel per item.  The
// reference (main.cu:125-145) instead gives each thread one pixel and loops
// all its samples, so a warp waits for its longest path at every sample.
// Per path segment: stackless BVH walk over the flattened objects (the
// reference walks a pointer tree of virtual hittables), deferred hit record
// of the winner, then texture lookup and scatter.
#include <cstdlib>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <type_traits>

#include "rtmi_internal.h"
#include "rtmi_nw_internal.h"
#include "rtmi_nw_path.h"

namespace rtmi {
namespace nw {

struct Args {
  Cam<float> cam;
  float time0, time1;
  int32_t W, H, s_end, max_depth;  // s_end: one past the launch's last sample, s_base + its sample count
  uint64_t seed;
  int32_t row0, row_step, nrows_valid;
  int32_t tiles_x, tiles, chunk, nch, n_items;
  // first sample of the launch (a progressive pass, rt_nw_render_pass; 0 in a plain render): item c of a tile
  // takes the samples s_base + c * chunk + [0, ns).  Wave-uniform: one scalar add per item.
  int32_t s_base;
};

// The adaptive form's work list (rt_nw_adapt_pass, DESIGN.md §9 "Adaptive sampling"): the pass's active tiles and,
// per active tile, its pixel set as a mask (bit ly * 8 + lx); the samples each pixel holds (read, never written, by
// the render kernels: adapt_advance_kernel adds the pass's count afterwards) and the second-moment sums.  Item
// `it` renders tile tiles[it / nch]; Args' tiles is the list's length, s_base 0 and s_end the pass's sample count.
struct AdaptArgs {
  const int32_t *__restrict__ tiles;
  const unsigned long long *__restrict__ masks;
  const int32_t *__restrict__ n;     // [nrows][W]
  unsigned long long *__restrict__ m2;  // [nrows][W]
};

// Two kernel shapes, the same per-path arithmetic (bit-identical images):
//  * persistent (default when the scene fits in LDS): one 16-wave block per
//    CU stages the BVH nodes — and the objects, when they fit too — into LDS
//    once for the whole launch; its waves pull work items from a global
//    counter, so no wave waits for a slow item of another;
//  * grid: one wave per work item in 4-wave blocks, nodes in LDS when they
//    fit the per-block budget (several blocks per CU), else in global memory.
// Measured (profiles/r01/nw): 4-wave grid blocks beat 8-wave ones (a block's
// LDS stays allocated until its slowest item ends), LDS nodes +23% and LDS
// objects +13% on the motion-blur scene.
#ifndef RTMI_NW_WAVES
#define RTMI_NW_WAVES 4
#endif
#ifndef RTMI_NW_LDS_KB
#define RTMI_NW_LDS_KB 34
#endif
#ifndef RTMI_NW_PERSIST
#define RTMI_NW_PERSIST 1
#endif
#ifndef RTMI_NW_LDS_OBJS
#define RTMI_NW_LDS_OBJS 1
#endif
constexpr int kWaves = RTMI_NW_WAVES;                         // grid kernel: waves per block
constexpr size_t kLdsBudget = size_t(RTMI_NW_LDS_KB) * 1024;  // grid kernel: staged bytes per block
constexpr int kPWaves = 16;                                   // persistent kernel: waves per block (one per CU)
// spheres-only instantiation of the persistent kernel: waves per block and
// the minimum waves per SIMD it is compiled for (VGPR budget 512 / per_eu).
// Motion-blur scene 1200x800x500 (profiles/r02/ab_nw_spheres_only/): general
// kernel 100.6 ms; spheres-only at 89 VGPRs (4 waves per SIMD) 79.2;
// 8-wave blocks at 6 per SIMD (80 VGPRs, 7 spilled) 63.8; 16- or 8-wave
// blocks at 8 per SIMD (64 VGPRs, spills) 60.4-60.5
#ifndef RTMI_NW_SIMPLE_WAVES
#define RTMI_NW_SIMPLE_WAVES 16
#endif
#ifndef RTMI_NW_SIMPLE_PER_EU
#define RTMI_NW_SIMPLE_PER_EU 8
#endif
template <bool S> constexpr int persist_waves() { return S ? RTMI_NW_SIMPLE_WAVES : kPWaves; }
// minimum waves per SIMD of the general persistent kernel's BVH
// instantiations: 8 (64 VGPRs, spills) lets two 16-wave blocks share a CU
// when the staged bytes allow it.  Final scene at 1024 spp
// (profiles/r02/ab_nw_occupancy/): nodes + objects in LDS, one block per CU
// (100 VGPRs) 1 062 ms; objects in global memory, one block 1 185; objects
// in global memory, two blocks at 64 VGPRs 1 009-1 013.
#ifndef RTMI_NW_PERSIST_PER_EU
#define RTMI_NW_PERSIST_PER_EU 8
#endif
// Dynamic LDS budgets of the persistent kernel, derived from its static LDS
// (the waves' accumulators and the camera, rounded up to the allocation
// granule): staged bytes (nodes, and objects when they fit) that leave room
// for two blocks per CU, and for one (160 KB LDS per CU).  The launch path
// also checks the kernel's actual static size (hipFuncGetAttributes), so a
// new __shared__ variable cannot silently push a block past the CU.
// Scenes with placements of shared meshes (TRI = 3, the two-level walk
// hit_world_nw_inst): minimum waves per SIMD of its persistent instantiations.
// The walk keeps the local ray, its inverses and the triangle constants beside
// the world ray's: 128 VGPRs without scratch at 4 waves per SIMD (one 16-wave
// block per CU), 64 VGPRs with ~185 spilled at 8 (two blocks).  The bottom
// level is a chain of dependent global loads, and the waves that hide them win
// once the meshes are large: a 16 x 16 field of an 81 920-triangle mesh at 800
// x 800 x 64 renders in 157.5 ms at 4 and 123.7 ms at 8, of a 5 120-triangle
// one in 81.8 and 74.6; only the 4 x 4 field of the small mesh prefers 4 (49.0
// against 50.1).  profiles/instancing/README.md
#ifndef RTMI_NW_INST_PER_EU
#define RTMI_NW_INST_PER_EU 8
#endif
// Scenes with a moving placement (TRI = 4: the same walk, the placement's
// offset formed at the ray's time on entering it).  TRI = 3's choice does not
// carry over: compiled for 8 waves per SIMD (64 VGPRs, 191-229 spilled) the
// persistent kernels render the fields of profiles/motion/README.md in 74.0 /
// 110.7 / 123.9 / 186.6 ms (every placement moving; 65.4 / 101.8 / 109.0 / 172.4
// with every placement under a move at rest, against 49.9 / 74.5 / 84.5 / 123.9
// of the static TRI = 3 build of the same fields), compiled for 4 (128 VGPRs,
// no scratch, one 16-wave block per CU) in 57.9 / 88.1 / 111.1 / 170.0 ms (at
// rest 48.4 / 81.1 / 93.5 / 156.9).  Why the 8-wave build loses that much to
// TRI = 3's at the same size and spill count was not found.
#ifndef RTMI_NW_MOVE_PER_EU
#define RTMI_NW_MOVE_PER_EU 4
#endif
// Scenes with an affine placement (TRI = 5: TRI = 4's walk with the 3x3 entry
// for the placements flagged affine).  Like TRI = 4 and unlike TRI = 3:
// compiled for 8 waves per SIMD (64 VGPRs, 226-228 spilled) the persistent
// kernels render the fields of profiles/affine/README.md in 88.8 / 130.9 / 169.9
// / 244.7 ms (every placement an affine map of the rotate_y field's geometry),
// compiled for 4 (128 VGPRs, no scratch) in 54.1 / 90.7 / 125.7 / 212.0 ms.
#ifndef RTMI_NW_AFFINE_PER_EU
#define RTMI_NW_AFFINE_PER_EU 4
#endif
constexpr int affine_per_eu(int tri) { return tri == 5 ? RTMI_NW_AFFINE_PER_EU : RTMI_NW_MOVE_PER_EU; }
// hit_world_nw_inst's / make_rec_inst's mode of a family: 0 static placements, 1 some move, 2 some are affine
constexpr int inst_mode(int tri) { return tri == 5 ? 2 : tri == 4 ? 1 : 0; }
constexpr size_t kCuLds = 160 * 1024;
constexpr size_t kPStaticLds = (sizeof(unsigned long long) * 3 * 64 * kPWaves + 23 * sizeof(float) + 255) / 256 * 256;
constexpr size_t kPTwoBlockBudget = kCuLds / 2 - kPStaticLds;
constexpr size_t kPLdsBudget = kCuLds - kPStaticLds;
// ... of the adaptive kernels (ADAPT; rt_nw_adapt_pass): a wave's static LDS is four accumulators (the three colour
// sums and the second moment) and its 64-entry pixel list, 2.25 KB against 1.5 KB, so their budgets are their own
constexpr size_t kAdaptWaveLds = sizeof(unsigned long long) * 4 * 64 + sizeof(uint32_t) * 64;
constexpr size_t kPStaticLdsA = (kAdaptWaveLds * kPWaves + 23 * sizeof(float) + 255) / 256 * 256;
constexpr size_t kPTwoBlockBudgetA = kCuLds / 2 - kPStaticLdsA;
constexpr size_t kPLdsBudgetA = kCuLds - kPStaticLdsA;
constexpr size_t kLdsBudgetA = kLdsBudget - (kAdaptWaveLds - sizeof(unsigned long long) * 3 * 64) * kWaves;  // grid kernel: per block

// RTMI_NW_PHASES builds (analysis only): wave-level cycles (s_memtime) of a
// work item's loop passes: [0] closest hit, [1] hit record + texture +
// scatter, [2] accumulation + regeneration, [3] whole item; read with
// rt_nw_debug_phases.
#ifndef RTMI_NW_PHASES
#define RTMI_NW_PHASES 0
#endif
#if RTMI_NW_PHASES
__device__ unsigned long long g_nw_phase[4];
#endif
#if RTMI_STATS
// RTMI_STATS build: executed work of the launches since the last
// rt_nw_debug_counters call — FLOP, node visits, object tests, cell steps
__device__ unsigned long long g_nw_stats[4];
#endif

// NaN -> 0, clamped to [0, 64]: as rtmi_device.hip to_fixed (and the oracle)
__device__ __forceinline__ int64_t fixed(float c) {
  const float g = c == c ? __builtin_amdgcn_fmed3f(c, 0.0f, 64.0f) : 0.0f;  // branch-free guard
  const uint32_t hi = uint32_t(g);
  const uint32_t lo = uint32_t((g - float(hi)) * 4294967296.0f);
  return int64_t((uint64_t(hi) << 32) | lo);
}

// The camera, shutter and image size in LDS (23 floats), read at each
// regeneration: the kernel's scalar registers otherwise overflow and the
// compiler parks them in VGPR lanes (v_readlane at every regeneration), as in
// the RTIOW kernel.  Staged before stage_scene's barrier.
__device__ __forceinline__ void stage_camera(float *cl, const Args &a) {
  const unsigned t = threadIdx.x;
  if (t < 23) {
    float v;
    switch (t / 3) {
      case 0: v = (&a.cam.origin.x)[t % 3]; break;
      case 1: v = (&a.cam.llc.x)[t % 3]; break;
      case 2: v = (&a.cam.hor.x)[t % 3]; break;
      case 3: v = (&a.cam.ver.x)[t % 3]; break;
      case 4: v = (&a.cam.u.x)[t % 3]; break;
      case 5: v = (&a.cam.v.x)[t % 3]; break;
      default:
        v = t == 18 ? a.cam.lens : t == 19 ? a.time0 : t == 20 ? a.time1 - a.time0 : t == 21 ? float(a.W) : float(a.H);
        break;
    }
    cl[t] = v;
  }
}

template <bool LDS_NODES, bool LDS_OBJS, bool GRID>
__device__ __forceinline__ void stage_scene(const View &sc) {
  if constexpr (GRID) {  // objects, insertion indices, cell starts, refs, brute-force list (nw_grid_lds_bytes)
    const float4 *src = reinterpret_cast<const float4 *>(sc.obj);
    for (int i = threadIdx.x; i < 3 * sc.nobj; i += blockDim.x) nw_nodes_lds[i] = src[i];
    int32_t *ids = reinterpret_cast<int32_t *>(nw_nodes_lds + 3 * sc.nobj);
    for (int i = threadIdx.x; i < sc.nobj; i += blockDim.x) ids[i] = sc.obj_id[i];
    uint16_t *u = reinterpret_cast<uint16_t *>(ids + sc.nobj);
    const int nstart = sc.grid.ncells + 1;
    for (int i = threadIdx.x; i < nstart; i += blockDim.x) u[i] = sc.grid.cell_start[i];
    for (int i = threadIdx.x; i < sc.grid.nrefs; i += blockDim.x) u[nstart + i] = sc.grid.refs[i];
    int32_t *big = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(u) + ((size_t(nstart) + sc.grid.nrefs) * 2 + 3) / 4 * 4);
    for (int i = threadIdx.x; i < sc.nbig; i += blockDim.x) big[i] = sc.gbig[i];
    __syncthreads();
  } else if constexpr (LDS_NODES) {  // BVH nodes (lo[], hi[]), then objects and their insertion indices
    for (int i = threadIdx.x; i < sc.nnodes; i += blockDim.x) {
      nw_nodes_lds[i] = sc.nlo[i];
      nw_nodes_lds[sc.nnodes + i] = sc.nhi[i];
    }
    if constexpr (LDS_OBJS) {
      const float4 *src = reinterpret_cast<const float4 *>(sc.obj);
      float4 *dst = nw_nodes_lds + 2 * sc.nnodes;
      for (int i = threadIdx.x; i < 3 * sc.nobj; i += blockDim.x) dst[i] = src[i];
      int32_t *ids = reinterpret_cast<int32_t *>(dst + 3 * sc.nobj);
      for (int i = threadIdx.x; i < sc.nobj; i += blockDim.x) ids[i] = sc.obj_id[i];
    }
    __syncthreads();
  }
}

// One work item = (8x8 tile, <= chunk samples) on one wave: lanes pull
// (pixel, sample) jobs from the item's queue and regenerate paths as theirs
// end; sums in the wave's LDS accumulator, then one global add per pixel.
// ADAPT (always CHUNKED; rt_nw_adapt_pass): the item's tile comes from the list of active tiles and its pixels
// are the set bits of that tile's mask.  The lanes whose bit is set rank themselves and write pixel | n[pixel] <<
// 8 into the wave's list (n < 2^20 fits); job q then goes to list entry q % nv (nv = the mask's popcount), sample
// n[pixel] + s0 + q / nv, so pixels of one tile may start at different samples and a sparse tile's lanes take
// several samples of one pixel side by side (nv * ns jobs: a tile with one active pixel runs ns lanes).  A path that ends also adds l^2, l = (fx + fy + fz) >> 18, to a
// fourth accumulator (acc[3], flushed into ad.m2).  acc is indexed by the pixel's bit ly * 8 + lx here, by ly * vw
// + lx otherwise.
template <bool CHUNKED, bool LDS_NODES, bool LDS_OBJS, bool GRID, bool S = false, int TRI = 0, bool ADAPT = false>
__device__ __forceinline__ void run_item(const View &sc, const Args &a, int item, int lane,
                                         unsigned long long (&acc)[ADAPT ? 4 : 3][64], unsigned long long *__restrict__ accum,
                                         float *__restrict__ out, unsigned &nseg, const float *cl,
                                         const AdaptArgs &ad = AdaptArgs{}, uint32_t *list = nullptr) {
  static_assert(!ADAPT || CHUNKED, "the adaptive form adds into an accumulator");
  const int slot = item / a.nch;  // the tile (ADAPT: its place in the list of active tiles)
  const int tile = ADAPT ? ad.tiles[slot] : slot;
  const int s0 = a.s_base + (item - slot * a.nch) * a.chunk;
  const int ns = min(a.chunk, a.s_end - s0);  // (the job decode below works on the item-local q < nv * ns)
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int x0 = tx * 8, y0 = ty * 8;
  const int vw = min(8, a.W - x0), vh = min(8, a.nrows_valid - y0);
  const unsigned long long pmask = ADAPT ? ad.masks[slot] : 0ull;  // wave-uniform
  const int nv = ADAPT ? int(__popcll(pmask)) : vw * vh;
  const int nq = nv * ns;

  acc[0][lane] = 0;
  acc[1][lane] = 0;
  acc[2][lane] = 0;
  if constexpr (ADAPT) {
    acc[3][lane] = 0;
    if ((pmask >> lane) & 1ull) {  // (the host sets bits of the tile's valid pixels only)
      const int rank = __builtin_amdgcn_mbcnt_hi(unsigned(pmask >> 32), __builtin_amdgcn_mbcnt_lo(unsigned(pmask), 0u));
      const size_t op = size_t(y0 + (lane >> 3)) * size_t(a.W) + size_t(x0 + (lane & 7));
      list[rank] = uint32_t(lane) | uint32_t(ad.n[op]) << 8;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }

  V o, d, T;
  float time = 0.f;
  // the path's pixel in the tile (bits 24..29) and its depth (bits 0..23;
  // max_depth < 2^24 is checked on the host) in one register
  int pxd = 0;
  Xoro rng;
  // job q -> pixel q % nv, sample s0 + q / nv (s0 includes the launch's s_base); camera ray main.cu:139-141.
  // Grid kernels: q / d = umulhi(2q, ceil(2^31 / d)), exact for d <= 64,
  // q < 2^25 (the RTIOW kernel's job decode, tests/test_kernel_arith.py;
  // chunk <= 65535 keeps q < 2^22) — a multiply instead of the 32-bit division
  // expansion (motion blur 59.5 -> 58.1 ms); the BVH kernel keeps the division
  // (its two multipliers cost more registers than they save: final scene
  // 283.6 -> 286.2 ms at 256 spp, profiles/r03/ab_nw_jobdiv.txt)
  constexpr bool kMulDiv = GRID;
  const uint32_t m_nv = 0x7FFFFFFFu / uint32_t(max(nv, 1)) + 1u, m_vw = 0x7FFFFFFFu / uint32_t(vw) + 1u;
  auto start = [&](int q) {
    const int qs = kMulDiv ? int(__umulhi(uint32_t(q) << 1, m_nv)) : q / nv;
    int s = s0 + qs;
    int px = q - qs * nv;
    int ly, lx;
    if constexpr (ADAPT) {  // the list entry: the pixel's bit and the samples it holds already
      const uint32_t e = list[px];
      px = int(e & 63u);
      s += int(e >> 8);
      ly = px >> 3;
      lx = px & 7;
    } else {
      ly = kMulDiv ? int(__umulhi(uint32_t(px) << 1, m_vw)) : px / vw;
      lx = px - ly * vw;
    }
    const int i = x0 + lx;
    const int j = a.row0 + (y0 + ly) * a.row_step;
    rng.init(a.seed, uint64_t(j) * uint64_t(a.W) + uint64_t(i), uint32_t(s));
    float ju, jv;
    rng.pair(ju, jv);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");  // read here, not hoisted out of the loop
    const float u = (float(i) + ju) / cl[21];
    const float v = (float(j) + jv) / cl[22];
    Cam<float> cm;
    cm.origin = mk(cl[0], cl[1], cl[2]);
    cm.llc = mk(cl[3], cl[4], cl[5]);
    cm.hor = mk(cl[6], cl[7], cl[8]);
    cm.ver = mk(cl[9], cl[10], cl[11]);
    cm.u = mk(cl[12], cl[13], cl[14]);
    cm.v = mk(cl[15], cl[16], cl[17]);
    cm.lens = cl[18];
    get_ray<true, float>(cm, u, v, rng, o, d);
    time = __builtin_fmaf(rng.uni(), cl[20], cl[19]);  // camera.h:75-79
    T = mk(1.f, 1.f, 1.f);
    pxd = px << 24;
  };

#if RTMI_NW_PHASES
  unsigned long long ph[4] = {0, 0, 0, 0}, pa = 0, pb = 0;
  const unsigned long long p_start = __builtin_amdgcn_s_memtime();
#endif
  NwCount cnt{0, 0, 0, 0};
  bool active = lane < nq;
  if (active) start(lane);
  int next = 64;
  for (;;) {
    const unsigned long long live = __ballot(active);
    if (live == 0) break;
    nseg = unsigned(__builtin_amdgcn_readfirstlane(int(nseg + unsigned(__popcll(live)))));
    bool done = false;
    V col = mk(0.f, 0.f, 0.f);
#if RTMI_NW_PHASES
    pa = __builtin_amdgcn_s_memtime();
#endif
    if (active) {
      const uint64_t seg_key = !S && sc.has_media ? rng.next() : 0ull;
      float t;
      int face;
      int32_t sub = -1;  // the winner's pool slot when it is a placement's triangle (TRI = 3, 4)
      const int32_t k = TRI >= 3 ? hit_world_nw_inst<LDS_NODES, LDS_OBJS, inst_mode(TRI)>(sc, o, d, time, seg_key, t, face, sub, &cnt)
                        : GRID   ? hit_world_nw_grid<S, TRI>(sc, o, d, time, seg_key, t, face, &cnt)
                                 : hit_world_nw<LDS_NODES, LDS_OBJS, TRI>(sc, o, d, time, seg_key, t, face, &cnt);
#if RTMI_NW_PHASES
      pb = __builtin_amdgcn_s_memtime();
#endif
      if (k < 0) {  // background main.cu:92-99
        col = mk(T.x * sc.bg[0], T.y * sc.bg[1], T.z * sc.bg[2]);
        done = true;
      } else {
        const Rec rec = TRI >= 3 && k < sc.nobj ? make_rec_inst<inst_mode(TRI)>(sc, k, sub, o, d, time, t, face)
                        : S || k < sc.nobj      ? make_rec<S, TRI>(sc, sc.obj[k], o, d, time, t, face, attr_view_of(sc), k)
                                                : make_rec_medium(sc, sc.med[k - sc.nobj], o, d, time);
        const Mat m = sc.mat[rec.mat];
        V at, nd;
        if (m.kind == kDiffuseLight) {  // emitted, no scatter: main.cu:76-90
          col = mul3(T, tex_value<S>(sc, m.tex, rec.u, rec.v, rec.p));
          done = true;
        } else if (!scatter_nw<S>(sc, rec, d, rng, at, nd)) {
          done = true;  // absorbed: emitted() = 0
        } else {
          T = mul3(T, at);
          o = rec.p;
          d = nd;
          if ((++pxd & 0xFFFFFF) >= a.max_depth) {  // main.cu:100: the background, unattenuated
            col = mk(sc.bg[0], sc.bg[1], sc.bg[2]);
            done = true;
          }
        }
      }
    }
#if RTMI_NW_PHASES
    const unsigned long long pc = __builtin_amdgcn_s_memtime();
    pb = __shfl(pb, __builtin_ctzll(__ballot(active)));  // (set by the lanes that ran the hit)
    ph[0] += pb - pa;
    ph[1] += pc - pb;
#endif
    const unsigned long long m = __ballot(done);
    if (m) {
      if (done) {
        const int px = pxd >> 24;
        if constexpr (ADAPT) {  // ... and the channel sum in units of 2^-14 (< 2^22), squared
          const int64_t fx = fixed(col.x), fy = fixed(col.y), fz = fixed(col.z);
          atomicAdd(&acc[0][px], (unsigned long long)fx);
          atomicAdd(&acc[1][px], (unsigned long long)fy);
          atomicAdd(&acc[2][px], (unsigned long long)fz);
          const unsigned long long l = (unsigned long long)(fx + fy + fz) >> 18;
          atomicAdd(&acc[3][px], l * l);
        } else {  // (the statement form the existing kernels were compiled from: their code depends on it)
          atomicAdd(&acc[0][px], (unsigned long long)fixed(col.x));
          atomicAdd(&acc[1][px], (unsigned long long)fixed(col.y));
          atomicAdd(&acc[2][px], (unsigned long long)fixed(col.z));
        }
        const int rank = __builtin_amdgcn_mbcnt_hi(unsigned(m >> 32), __builtin_amdgcn_mbcnt_lo(unsigned(m), 0u));
        const int q = next + rank;
        if (q < nq) start(q);
        else active = false;
      }
      next = __builtin_amdgcn_readfirstlane(next + int(__popcll(m)));
    }
#if RTMI_NW_PHASES
    ph[2] += __builtin_amdgcn_s_memtime() - pc;
#endif
  }
#if RTMI_NW_PHASES
  ph[3] = __builtin_amdgcn_s_memtime() - p_start;
  if (lane == __builtin_ctzll(__ballot(1)))
    for (int q = 0; q < 4; ++q) atomicAdd(&g_nw_phase[q], ph[q]);
#endif
#if RTMI_STATS
  atomicAdd(&g_nw_stats[0], cnt.flop);
  atomicAdd(&g_nw_stats[1], (unsigned long long)cnt.nodes);
  atomicAdd(&g_nw_stats[2], (unsigned long long)cnt.objects);
  atomicAdd(&g_nw_stats[3], (unsigned long long)cnt.cells);
#else
  (void)cnt;
#endif
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if constexpr (ADAPT) {
    if ((pmask >> lane) & 1ull) {
      const size_t op = size_t(y0 + (lane >> 3)) * size_t(a.W) + size_t(x0 + (lane & 7));
      for (int c = 0; c < 3; ++c) atomicAdd(&accum[op * 3 + c], acc[c][lane]);
      atomicAdd(&ad.m2[op], acc[3][lane]);
    }
  } else if (lane < nv) {
    const int ly = lane / vw, lx = lane - ly * vw;
    const size_t o3 = (size_t(y0 + ly) * size_t(a.W) + size_t(x0 + lx)) * 3;
    for (int c = 0; c < 3; ++c) {
      const unsigned long long v = acc[c][lane];
      if constexpr (CHUNKED) atomicAdd(&accum[o3 + c], v);
      else out[o3 + c] = float((long long)v) * 0x1p-32f;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void add_segments(unsigned nseg, int lane, unsigned long long *segments) {
  if (lane == 0) atomicAdd(segments, (unsigned long long)nseg);  // the wave's world.hit calls (wave-uniform)
}

// TRI: the scene holds no triangle (0), triangles (1), triangles with
// attribute records (2; hit_object, make_rec), placements of shared meshes (3; hit_world_nw_inst: BVH
// shapes only, such a scene has no uniform grid), placements of which some move (4; the same walk with
// the moving placements' offsets formed at the ray's time), placements of which some are affine (5; the
// same walk with the 3x3 entry of rtmi_nw_path.h to_local_affine)
template <bool CHUNKED, bool LDS_NODES, bool LDS_OBJS, bool GRID, int TRI = 0>
__global__ __launch_bounds__(64 * kWaves) void render_kernel(View sc, Args a, unsigned long long *__restrict__ accum,
                                                             float *__restrict__ out,
                                                             unsigned long long *__restrict__ segments) {
  __shared__ unsigned long long acc[kWaves][3][64];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * kWaves + wave;
  __shared__ float cam_lds[23];
  stage_camera(cam_lds, a);
  if constexpr (!LDS_NODES && !GRID) __syncthreads();  // (stage_scene's barrier covers the others)
  stage_scene<LDS_NODES, LDS_OBJS, GRID>(sc);  // block barrier inside: before any wave leaves
  if (item >= a.n_items) return;         // wave-uniform
  unsigned nseg = 0;
  run_item<CHUNKED, LDS_NODES, LDS_OBJS, GRID, false, TRI>(sc, a, item, lane, acc[wave], accum, out, nseg, cam_lds);
  add_segments(nseg, lane, segments);
}

#ifndef RTMI_NW_PERSIST_GRID_PER_EU
#define RTMI_NW_PERSIST_GRID_PER_EU 1
#endif
// minimum waves per SIMD a persistent kernel (and its adaptive twin) is compiled for
constexpr int persist_per_eu(bool s, bool grid, int tri) {
  return s ? RTMI_NW_SIMPLE_PER_EU : grid ? RTMI_NW_PERSIST_GRID_PER_EU : tri >= 4 ? affine_per_eu(tri) : tri == 3 ? RTMI_NW_INST_PER_EU : RTMI_NW_PERSIST_PER_EU;
}
template <bool CHUNKED, bool LDS_OBJS, bool GRID, bool S = false, int TRI = 0>
__global__ __launch_bounds__(64 * persist_waves<S>(), persist_per_eu(S, GRID, TRI)) void render_persistent(View sc, Args a,
                                                                  unsigned long long *__restrict__ accum,
                                                                  float *__restrict__ out,
                                                                  unsigned long long *__restrict__ segments,
                                                                  unsigned *__restrict__ counter) {
  __shared__ unsigned long long acc[persist_waves<S>()][3][64];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  __shared__ float cam_lds[23];
  stage_camera(cam_lds, a);
  stage_scene<true, LDS_OBJS, GRID>(sc);  // (its barrier covers the camera)
  unsigned nseg = 0;
  for (;;) {  // every wave leaves when the counter passes n_items
    unsigned it = 0;
    if (lane == 0) it = atomicAdd(counter, 1u);
    it = __builtin_amdgcn_readfirstlane(__shfl(it, 0));
    if (int(it) >= a.n_items) break;
    run_item<CHUNKED, true, LDS_OBJS, GRID, S, TRI>(sc, a, int(it), lane, acc[wave], accum, out, nseg, cam_lds);
  }
  add_segments(nseg, lane, segments);
}

// The adaptive twins (rt_nw_adapt_pass): the same shapes with run_item's ADAPT form, kernels of their own so that
// the ones above keep their code, registers and LDS.  Per wave four accumulators and the pixel list.
template <bool LDS_NODES, bool LDS_OBJS, bool GRID, int TRI = 0>
__global__ __launch_bounds__(64 * kWaves) void render_kernel_adapt(View sc, Args a, AdaptArgs ad,
                                                                   unsigned long long *__restrict__ accum,
                                                                   unsigned long long *__restrict__ segments) {
  __shared__ unsigned long long acc[kWaves][4][64];
  __shared__ uint32_t list[kWaves][64];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * kWaves + wave;
  __shared__ float cam_lds[23];
  stage_camera(cam_lds, a);
  if constexpr (!LDS_NODES && !GRID) __syncthreads();  // (stage_scene's barrier covers the others)
  stage_scene<LDS_NODES, LDS_OBJS, GRID>(sc);  // block barrier inside: before any wave leaves
  if (item >= a.n_items) return;         // wave-uniform
  unsigned nseg = 0;
  run_item<true, LDS_NODES, LDS_OBJS, GRID, false, TRI, true>(sc, a, item, lane, acc[wave], accum, nullptr, nseg, cam_lds, ad, list[wave]);
  add_segments(nseg, lane, segments);
}

template <bool LDS_OBJS, bool GRID, bool S = false, int TRI = 0>
__global__ __launch_bounds__(64 * persist_waves<S>(), persist_per_eu(S, GRID, TRI)) void render_persistent_adapt(View sc, Args a, AdaptArgs ad,
                                                                  unsigned long long *__restrict__ accum,
                                                                  unsigned long long *__restrict__ segments,
                                                                  unsigned *__restrict__ counter) {
  __shared__ unsigned long long acc[persist_waves<S>()][4][64];
  __shared__ uint32_t list[persist_waves<S>()][64];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  __shared__ float cam_lds[23];
  stage_camera(cam_lds, a);
  stage_scene<true, LDS_OBJS, GRID>(sc);  // (its barrier covers the camera)
  unsigned nseg = 0;
  for (;;) {  // every wave leaves when the counter passes n_items
    unsigned it = 0;
    if (lane == 0) it = atomicAdd(counter, 1u);
    it = __builtin_amdgcn_readfirstlane(__shfl(it, 0));
    if (int(it) >= a.n_items) break;
    run_item<true, true, LDS_OBJS, GRID, S, TRI, true>(sc, a, int(it), lane, acc[wave], accum, nullptr, nseg, cam_lds, ad, list[wave]);
  }
  add_segments(nseg, lane, segments);
}

// After an adaptive pass, on its stream: n[p] += s_count for the pass's active pixels (several items of a tile read
// n during the pass, so the render kernel cannot advance it).  One 64-thread block per active tile.
__global__ __launch_bounds__(64) void adapt_advance_kernel(const int32_t *__restrict__ tiles,
                                                           const unsigned long long *__restrict__ masks, int32_t *__restrict__ n,
                                                           int32_t W, int32_t tiles_x, int32_t s_count) {
  const int tile = tiles[blockIdx.x];
  const int lane = threadIdx.x;
  if (!((masks[blockIdx.x] >> lane) & 1ull)) return;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  n[size_t(ty * 8 + (lane >> 3)) * size_t(W) + size_t(tx * 8 + (lane & 7))] += s_count;
}

// rt_nw_adapt_resolve: per-pixel means float(double(sum) * 2^-32 / n), 0 where n = 0
__global__ void adapt_resolve_kernel(const unsigned long long *__restrict__ sum, const int32_t *__restrict__ n,
                                     float *__restrict__ out, size_t npix) {
  const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= npix) return;
  const int32_t k = n[i];
  for (int c = 0; c < 3; ++c)
    out[3 * i + c] = k > 0 ? float(double((long long)sum[3 * i + c]) * 0x1p-32 / double(k)) : 0.0f;
}

// The walks of the validation kernels below, one instantiation each: the BVH from global memory; the uniform grid
// staged in LDS as the grid kernels stage it; the two-level walk of a scene with placements of shared meshes
// (hit_world_nw_inst's modes: static, some move, some are affine), nodes and records in global memory.
enum Walk { kWalkBvh, kWalkGrid, kWalkInst, kWalkMove, kWalkAffine, kWalks };

// closest hit of one ray through WALK (TRI: the triangle code of the one-level walks; sub: the winner's pool slot
// when it is a placement's triangle), the winner's insertion index and its hit record
template <int WALK, int TRI>
__device__ __forceinline__ int32_t walk_closest(const View &sc, const V &o, const V &d, float time, uint64_t key, float &t,
                                                int &face, int32_t &sub, NwCount *cnt) {
  if constexpr (WALK >= kWalkInst) return hit_world_nw_inst<false, false, WALK - kWalkInst>(sc, o, d, time, key, t, face, sub, cnt);
  else if constexpr (WALK == kWalkGrid) return hit_world_nw_grid<false, TRI>(sc, o, d, time, key, t, face, cnt);
  else return hit_world_nw<false, false, TRI>(sc, o, d, time, key, t, face, cnt);
}
template <int WALK> __device__ __forceinline__ int32_t walk_winner_id(const View &sc, int32_t k, int32_t sub) {
  if (k < 0) return -1;
  if (k >= sc.nobj) return sc.med_id[k - sc.nobj];
  if constexpr (WALK >= kWalkInst) return inst_winner_id(sc, k, sub);
  else return sc.obj_id[k];
}
template <int WALK>
__device__ __forceinline__ Rec walk_rec(const View &sc, int32_t k, int32_t sub, const V &o, const V &d, float time, float t,
                                        int face, int has_attr) {
  if (k >= sc.nobj) return make_rec_medium(sc, sc.med[k - sc.nobj], o, d, time);
  if constexpr (WALK >= kWalkInst) return make_rec_inst<WALK - kWalkInst>(sc, k, sub, o, d, time, t, face);
  else return make_rec<false, 2>(sc, sc.obj[k], o, d, time, t, face, has_attr ? attr_view_of(sc) : AttrView{nullptr, nullptr}, k);
}

// Debug (parity investigations): the segments of ONE camera sample (pixel
// i, j, sample s): per segment o.xyz, d.xyz, t, winner insertion index (as
// float bits) — the oracle's or_nw_trace records the same.
// has_attr: the scene has triangle attribute records (attr_view_of; the two-level walks do not read it).
template <int WALK>
__global__ void trace_kernel(View sc, Args a, int i, int j, int s, float *rec, int cap, int *n_out, int has_attr) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  Xoro rng;
  rng.init(a.seed, uint64_t(j) * uint64_t(a.W) + uint64_t(i), uint32_t(s));
  float ju, jv;
  rng.pair(ju, jv);
  V o, d;
  get_ray<true, float>(a.cam, (float(i) + ju) / float(a.W), (float(j) + jv) / float(a.H), rng, o, d);
  const float time = __builtin_fmaf(rng.uni(), a.time1 - a.time0, a.time0);
  int n = 0;
  // the walk's work counters (written only by the RTMI_STATS build, which
  // would otherwise dereference a null counter pointer here)
  NwCount tcnt{0, 0, 0, 0};
  for (int depth = 0; depth < a.max_depth && n < cap; ++depth) {
    const uint64_t seg_key = sc.has_media ? rng.next() : 0ull;
    float t;
    int face;
    int32_t sub = -1;
    const int32_t k = walk_closest<WALK, 2>(sc, o, d, time, seg_key, t, face, sub, &tcnt);
    float *r = rec + 12 * n++;
    r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z; r[6] = t;
    r[7] = __int_as_float(walk_winner_id<WALK>(sc, k, sub));
    r[8] = r[9] = r[10] = 0.f;
    r[11] = __int_as_float(face);
    if (k < 0) break;
    const Rec rc = walk_rec<WALK>(sc, k, sub, o, d, time, t, face, has_attr);
    r[8] = rc.n.x; r[9] = rc.n.y; r[10] = rc.n.z;
    const Mat m = sc.mat[rc.mat];
    V at, nd;
    if (m.kind == kDiffuseLight || !scatter_nw(sc, rc, d, rng, at, nd)) break;
    o = rc.p;
    d = nd;
  }
  *n_out = n;
}
// The ray time of that camera sample (rt_nw_debug_trace_t): trace_kernel's draws up to the time
__global__ void trace_time_kernel(Args a, int i, int j, int s, float *time_out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  Xoro rng;
  rng.init(a.seed, uint64_t(j) * uint64_t(a.W) + uint64_t(i), uint32_t(s));
  float ju, jv;
  rng.pair(ju, jv);
  V o, d;
  get_ray<true, float>(a.cam, (float(i) + ju) / float(a.W), (float(j) + jv) / float(a.H), rng, o, d);
  *time_out = __builtin_fmaf(rng.uni(), a.time1 - a.time0, a.time0);
}

__global__ void finalize_kernel(const unsigned long long *__restrict__ acc, float *__restrict__ out, size_t n) {
  const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) out[i] = float((long long)acc[i]) * 0x1p-32f;
}

// The rays and the outputs of rt_nw_debug_hits / rt_nw_debug_records, per ray
struct DebugRays {
  const float *rays;               // {o.xyz, d.xyz, time, -}
  const unsigned long long *keys;  // the segments' medium keys (null: 0)
  int32_t n, has_attr;             // has_attr: as trace_kernel's (records only)
  int32_t *id;                     // out: the winner's insertion index (-1: miss)
  float *t;
  int32_t *aux;                    // out: the box face (hits), the material (records)
  float *pnuv;                     // out, records only: {p.xyz, n.xyz, u, v}
};

// Closest hit of n given rays through the walk the renders use (validation: rt_nw_debug_hits).
template <int WALK> __global__ __launch_bounds__(256) void debug_hits_kernel(View sc, DebugRays q) {
  stage_scene<false, false, WALK == kWalkGrid>(sc);  // (grid: ends with the block barrier, before any thread leaves)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= q.n) return;
  const float *r = q.rays + 8 * size_t(i);
  const V o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
  NwCount cnt{0, 0, 0, 0};
  float t;
  int face;
  int32_t sub = -1;
  const int32_t k = walk_closest<WALK, 1>(sc, o, d, r[6], q.keys ? q.keys[i] : 0ull, t, face, sub, &cnt);
  q.id[i] = walk_winner_id<WALK>(sc, k, sub);
  q.t[i] = t;
  q.aux[i] = face;
}

// The hit record of n given rays (validation: rt_nw_debug_records): the
// closest hit as debug_hits_kernel resolves it, then the record a render makes
// of it (make_rec with the attribute path, make_rec_inst, make_rec_medium).  A miss: index -1, everything else zero.
template <int WALK> __global__ __launch_bounds__(256) void debug_records_kernel(View sc, DebugRays q) {
  stage_scene<false, false, WALK == kWalkGrid>(sc);  // (grid: ends with the block barrier, before any thread leaves)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= q.n) return;
  const float *r = q.rays + 8 * size_t(i);
  const V o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
  NwCount cnt{0, 0, 0, 0};
  float t;
  int face;
  int32_t sub = -1;
  const int32_t k = walk_closest<WALK, 2>(sc, o, d, r[6], q.keys ? q.keys[i] : 0ull, t, face, sub, &cnt);
  float *p = q.pnuv + 8 * size_t(i);
  if (k < 0) {
    q.id[i] = -1;
    q.t[i] = 0.0f;
    q.aux[i] = 0;
    for (int c = 0; c < 8; ++c) p[c] = 0.0f;
    return;
  }
  const Rec rc = walk_rec<WALK>(sc, k, sub, o, d, r[6], t, face, q.has_attr);
  q.id[i] = walk_winner_id<WALK>(sc, k, sub);
  q.t[i] = t;
  q.aux[i] = rc.mat;
  p[0] = rc.p.x; p[1] = rc.p.y; p[2] = rc.p.z;
  p[3] = rc.n.x; p[4] = rc.n.y; p[5] = rc.n.z;
  p[6] = rc.u; p[7] = rc.v;
}

// fixed()'s signed twin (the feature normals): NaN -> 0, clamped to [-64, 64], truncated toward zero
__device__ __forceinline__ int64_t fixed_signed(float c) {
  const float g = c == c ? __builtin_amdgcn_fmed3f(c, -64.0f, 64.0f) : 0.0f;
  const float m = __builtin_fabsf(g);
  const uint32_t hi = uint32_t(m);
  const uint32_t lo = uint32_t((m - float(hi)) * 4294967296.0f);
  const int64_t v = int64_t((uint64_t(hi) << 32) | lo);
  return g < 0.0f ? -v : v;
}
// ... and the one of a ray parameter: NaN -> 0, clamped to [0, 2^20]
__device__ __forceinline__ int64_t fixed_t(float c) {
  const float g = c == c ? __builtin_amdgcn_fmed3f(c, 0.0f, 1048576.0f) : 0.0f;
  const uint32_t hi = uint32_t(g);
  const uint32_t lo = uint32_t((g - float(hi)) * 4294967296.0f);
  return int64_t((uint64_t(hi) << 32) | lo);
}

// First-hit feature buffers (rt_nw_render_features, the denoiser's guides): one thread per pixel, which loops over
// the camera samples s < fspp.  Sample (i, j, s) is segment 0 of trace_kernel's (i, j, s), draw for draw; the sums
// are int64 fixed point per thread, so the means do not depend on anything but the samples.
struct FeatArgs {
  int32_t fspp, has_attr;
  float *out;  // {a.rgb, n.xyz, z, cov} per pixel
};
template <int WALK> __global__ __launch_bounds__(256) void features_kernel(View sc, Args a, FeatArgs f) {
  stage_scene<false, false, WALK == kWalkGrid>(sc);  // (grid: ends with the block barrier, before any thread leaves)
  const uint32_t px = blockIdx.x * blockDim.x + threadIdx.x;
  if (px >= uint32_t(a.W) * uint32_t(a.H)) return;
  const int j = int(px / uint32_t(a.W)), i = int(px - uint32_t(j) * uint32_t(a.W));
  int64_t sa[3] = {0, 0, 0}, sn[3] = {0, 0, 0}, st = 0;
  int32_t hits = 0;
  NwCount cnt{0, 0, 0, 0};
  for (int s = 0; s < f.fspp; ++s) {
    Xoro rng;
    rng.init(a.seed, uint64_t(j) * uint64_t(a.W) + uint64_t(i), uint32_t(s));
    float ju, jv;
    rng.pair(ju, jv);
    V o, d;
    get_ray<true, float>(a.cam, (float(i) + ju) / float(a.W), (float(j) + jv) / float(a.H), rng, o, d);
    const float time = __builtin_fmaf(rng.uni(), a.time1 - a.time0, a.time0);
    const uint64_t seg_key = sc.has_media ? rng.next() : 0ull;
    float t;
    int face;
    int32_t sub = -1;
    const int32_t k = walk_closest<WALK, 2>(sc, o, d, time, seg_key, t, face, sub, &cnt);
    V alb = mk(sc.bg[0], sc.bg[1], sc.bg[2]);
    if (k >= 0) {
      const Rec rc = walk_rec<WALK>(sc, k, sub, o, d, time, t, face, f.has_attr);
      const Mat m = sc.mat[rc.mat];
      alb = m.kind == kDielectric ? mk(1.0f, 1.0f, 1.0f) : tex_value<false>(sc, m.tex, rc.u, rc.v, rc.p);
      if (k < sc.nobj) {  // (a medium has no surface)
        sn[0] += fixed_signed(rc.n.x);
        sn[1] += fixed_signed(rc.n.y);
        sn[2] += fixed_signed(rc.n.z);
      }
      st += fixed_t(t);
      ++hits;
    }
    sa[0] += fixed(alb.x);
    sa[1] += fixed(alb.y);
    sa[2] += fixed(alb.z);
  }
  float *out = f.out + 8 * size_t(px);
  const double n = double(f.fspp);
  for (int c = 0; c < 3; ++c) {
    out[c] = float(double(sa[c]) * 0x1p-32 / n);
    out[3 + c] = float(double(sn[c]) * 0x1p-32 / n);
  }
  out[6] = hits > 0 ? float(double(st) * 0x1p-32 / double(hits)) : 0.0f;
  out[7] = float(double(hits) / n);
}

}  // namespace nw
}  // namespace rtmi

// ===========================================================================
// host side
// ===========================================================================
using namespace rtmi;
using namespace rtmi::nw;

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return set_error(RT_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

namespace {

struct Guard {
  int prev = -1;
  explicit Guard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    (void)hipSetDevice(dev);
  }
  ~Guard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// A device allocation that is freed on every path out of its scope
template <class T> struct DevBuf {
  T *p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t count) { return hipMalloc(reinterpret_cast<void **>(&p), count * sizeof(T)); }
  hipError_t upload(const T *src, size_t count) {  // allocated here
    const hipError_t e = alloc(count);
    return e != hipSuccess ? e : hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice);
  }
  hipError_t download(T *dst, size_t count) const { return hipMemcpy(dst, p, count * sizeof(T), hipMemcpyDeviceToHost); }
};

}  // namespace

struct rt_nw_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  DevObj *obj = nullptr;
  int32_t *obj_id = nullptr;
  Obj *med = nullptr;
  int32_t *med_id = nullptr;
  int32_t nmed = 0;
  Inst *inst = nullptr;
  Mat *mat = nullptr;
  Tex *tex = nullptr;
  float4 *pvec = nullptr;
  int32_t *pperm = nullptr;
  uint8_t *img = nullptr;
  Image *imgd = nullptr;
  float4 *nodes = nullptr;  // 2 * nnodes: lo[] then hi[]
  int32_t nobj = 0, nnodes = 0, ninst = 0, nmat = 0, ntex = 0;
  // uniform grid: descriptor, global arrays, brute-force list
  bool grid_ok = false;
  NwGridDesc grid{};
  int32_t grid_max_cell = 0;
  uint16_t *grid_cells = nullptr, *grid_refs = nullptr;
  int32_t *grid_big = nullptr;
  int32_t nbig = 0;
  int32_t accel = RT_NW_ACCEL_AUTO;
  float bg[3] = {0.f, 0.f, 0.f};
  int32_t has_media = 0;
  int32_t has_tri = 0;  // the kernels' TRI: 0 no triangle, 1 triangles, 2 triangles with attribute records,
                        // 3 placements of shared meshes (nobj, nnodes: the top level's), 4 placements of which
                        // at least one moves (rt_nw_move), 5 placements of which at least one is affine
                        // (rt_nw_transform)
  int32_t npool = 0, nbot = 0;  // TRI = 3: pool slots behind obj[nobj], bottom-level nodes behind nodes[2 * nnodes]
  int32_t nattr = 0;    // attribute records behind obj[nobj] (their locator behind obj_id[nobj]); 0: neither exists
  unsigned long long *accum = nullptr;
  size_t accum_cap = 0;
  float *scratch = nullptr;
  size_t scratch_cap = 0;
  // progressive passes (rt_nw_accum_reset / rt_nw_render_pass): an accumulator of its own, pass_W x pass_rows x 3
  // fixed-point sums holding pass_spp samples; accum above stays the scratch of a single render
  unsigned long long *pass_accum = nullptr;
  size_t pass_cap = 0;
  int32_t pass_W = 0, pass_rows = 0, pass_spp = 0;
  // adaptive sampling (rt_nw_adapt_*): a third accumulator, allocations of its own, adapt_W x adapt_rows pixels —
  // the colour sums as pass_accum holds them, the second-moment sums and the samples each pixel holds.  n_host
  // mirrors adapt_n (every change of n starts on the host), so a pass is checked against the 2^20 limit without a
  // device read.  adapt_list: the work lists of the last two passes, used in turn — a pass uploads its list in
  // stream order from the slot's host copy and waits only for the pass two back, which used the slot before.
  unsigned long long *adapt_sum = nullptr, *adapt_m2 = nullptr;
  int32_t *adapt_n = nullptr;
  size_t adapt_cap = 0;  // pixels allocated
  int32_t adapt_W = 0, adapt_rows = 0;
  std::vector<int32_t> adapt_n_host;
  struct AdaptList {
    int32_t *tiles = nullptr;
    unsigned long long *masks = nullptr;
    size_t cap = 0;
    std::vector<int32_t> host_tiles;  // (alive until the copy has run)
    std::vector<unsigned long long> host_masks;
    hipEvent_t done = nullptr;  // the end of the pass that used the slot
    bool used = false;
  } adapt_list[2];
  int adapt_slot = 0;
  DenoiseScratch denoise;  // the filter's images (rt_nw_denoise, rtmi_nw_denoise.hip)
  unsigned long long *segments = nullptr;
  unsigned *counter = nullptr;  // persistent kernel's work-item counter
  int32_t persist_blocks = 0;   // resident 16-wave blocks (CUs x blocks per CU), BVH kernels
  int32_t persist_blocks_grid = 0;  // the same for the general grid kernel
  // spheres-only scene (spheres and moving spheres, no instances or media,
  // solid and checker-of-solid textures): the persistent grid kernel's S
  // instantiation, with the other kinds' code compiled out (fewer VGPRs, more
  // waves); RTMI_NW_SIMPLE=0 turns it off (A/B and tests)
  bool simple = false;
  bool simple_ok = !(std::getenv("RTMI_NW_SIMPLE") && std::getenv("RTMI_NW_SIMPLE")[0] == '0');
  int32_t persist_blocks_simple = 0;
  // RTMI_NW_PERSIST=0: render with the one-shot grid-of-blocks kernels (A/B
  // and tests; the same image), read when the context is created
  bool persist_ok = !(std::getenv("RTMI_NW_PERSIST") && std::getenv("RTMI_NW_PERSIST")[0] == '0');
  int32_t cus = 0;  // compute units of the device
  // resident blocks per CU of a persistent launch, by (kernel, dynamic LDS
  // bytes): the occupancy query repeated with the bytes the launch stages
  std::vector<std::pair<std::pair<const void *, size_t>, int32_t>> occupancy;
  int32_t last_kernel[4] = {0, 0, 0, 0};  // rt_nw_ctx_last_kernel
  int32_t last_staging[2] = {0, 0};       // rt_nw_ctx_last_staging
  // samples per work item forced by RTMI_NW_CHUNK (A/B only; 0 = automatic),
  // read when the context is created
  int32_t env_chunk = std::getenv("RTMI_NW_CHUNK") ? std::atoi(std::getenv("RTMI_NW_CHUNK")) : 0;
  // the buffers above are shared by every render of the context: a render on
  // another stream first waits for the end of the last one (as rt_ctx)
  hipStream_t last_stream = nullptr;
  hipEvent_t last_done = nullptr;

  rt_nw_ctx() = default;
  rt_nw_ctx(const rt_nw_ctx &) = delete;
  rt_nw_ctx &operator=(const rt_nw_ctx &) = delete;
  ~rt_nw_ctx() {  // whatever has been made: rt_nw_ctx_destroy, and rt_nw_ctx_create's failure returns
    Guard g(device);
    if (stream) (void)hipStreamSynchronize(stream);
    for (void *p : {(void *)obj, (void *)obj_id, (void *)med, (void *)med_id, (void *)inst, (void *)mat, (void *)tex, (void *)pvec,
                    (void *)pperm, (void *)img, (void *)imgd, (void *)nodes, (void *)accum, (void *)scratch, (void *)segments,
                    (void *)counter, (void *)grid_cells, (void *)grid_refs, (void *)grid_big, (void *)pass_accum, (void *)adapt_sum,
                    (void *)adapt_m2, (void *)adapt_n, (void *)adapt_list[0].tiles, (void *)adapt_list[0].masks,
                    (void *)adapt_list[1].tiles, (void *)adapt_list[1].masks, denoise.p})
      if (p) (void)hipFree(p);
    for (auto &l : adapt_list)
      if (l.done) (void)hipEventDestroy(l.done);
    if (stream) (void)hipStreamDestroy(stream);
    if (last_done) (void)hipEventDestroy(last_done);
  }
};

namespace {

template <class T> int alloc_copy(T **p, const T *src, size_t count) {
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  const size_t n = count ? count : 1;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(p), n * sizeof(T));
  if (e != hipSuccess) return set_error(RT_ENOMEM, "hipMalloc(%zu B): %s", n * sizeof(T), hipGetErrorString(e));
  if (count && src) {
    e = hipMemcpy(*p, src, count * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) return set_error(RT_EHIP, "hipMemcpy: %s", hipGetErrorString(e));
  }
  return RT_OK;
}

Cam<float> camf(const rt_camera &c) {
  auto v = [](const double *p) { return mk(float(p[0]), float(p[1]), float(p[2])); };
  return Cam<float>{v(c.origin), v(c.lower_left_corner), v(c.horizontal), v(c.vertical), v(c.u), v(c.v),
                    float(c.lens_radius)};
}

View view_of(const rt_nw_ctx *c) {
  View v;
  v.obj = c->obj;
  v.obj_id = c->obj_id;
  v.med = c->med;
  v.med_id = c->med_id;
  v.nobj = c->nobj;
  v.nmed = c->nmed;
  v.inst = c->inst;
  v.mat = c->mat;
  v.tex = c->tex;
  v.perlin_vec = c->pvec;
  v.perlin_perm = c->pperm;
  v.image_px = c->img;
  v.image = c->imgd;
  v.nlo = c->nodes;
  v.nhi = c->nodes + c->nnodes;
  v.nnodes = c->nnodes;
  for (int i = 0; i < 3; ++i) v.bg[i] = c->bg[i];
  v.has_media = c->has_media;
  v.grid = c->grid;
  v.gbig = c->grid_big;
  v.nbig = c->nbig;
  return v;
}

// the camera's part of the kernels' arguments (everything else zero)
Args camera_args(const rt_nw_camera *cam, int32_t W, int32_t H, int32_t max_depth, uint64_t seed) {
  Args a{};
  a.cam = camf(cam->cam);
  a.time0 = float(cam->time0);
  a.time1 = float(cam->time1);
  a.W = W;
  a.H = H;
  a.max_depth = max_depth;
  a.seed = seed;
  return a;
}

// ---------------------------------------------------------------------------
// The kernel table (DESIGN.md §9 "The launch path"): what a launch stages and which instantiation runs, decided
// once.  Shape says what the kernel does with the scene; kernel_of maps (form, family, shape) to the instantiation
// and its block size.  The attribute check, the occupancy queries, the launch and the diagnostics
// (rt_nw_ctx_last_kernel, rt_nw_ctx_last_staging) all read these two, so they cannot disagree.
// ---------------------------------------------------------------------------
struct Shape {
  bool persist = false;    // the persistent kernels (one launch-long block per resident slot), else one wave per item
  bool grid = false;       // the uniform grid, staged whole (objects, cells, brute-force list), else the BVH
  bool simple = false;     // ... its spheres-only instantiation (persistent only)
  bool lds_nodes = false;  // BVH: the nodes are staged (the persistent kernels always stage them)
  bool lds_objs = false;   // BVH: ... and the objects beside them
  size_t lds = 0;          // the dynamic LDS bytes that go with the flags above
};

// The form of a launch: the kernel writes the floats itself (all samples of a tile in one item), adds fixed-point
// sums into an accumulator, or is the adaptive twin (which always adds).
enum Form { kOneShot, kChunked, kAdapt, kForms };
constexpr int kFamilies = 6;  // the kernels' TRI, rt_nw_ctx::has_tri

struct Kernel {
  const void *fn;
  int waves;  // per block
};

// The only place that names the render kernels.  T < 3: the families that may have a grid.
template <Form F, int T> Kernel kernel_ft(const Shape &s) {
  using Y = std::true_type;
  using N = std::false_type;
  auto persistent = [](auto objs, auto grid, auto simple) -> const void * {
    constexpr bool O = decltype(objs)::value, G = decltype(grid)::value, S = decltype(simple)::value;
    constexpr int TT = S ? 0 : T;  // (a spheres-only scene holds no triangle)
    if constexpr (F == kAdapt) return (const void *)render_persistent_adapt<O, G, S, TT>;
    else return (const void *)render_persistent<F == kChunked, O, G, S, TT>;
  };
  auto one_shot = [](auto nodes, auto objs, auto grid) -> const void * {
    constexpr bool Nd = decltype(nodes)::value, O = decltype(objs)::value, G = decltype(grid)::value;
    if constexpr (F == kAdapt) return (const void *)render_kernel_adapt<Nd, O, G, T>;
    else return (const void *)render_kernel<F == kChunked, Nd, O, G, T>;
  };
  if constexpr (T < 3) {
    if (s.simple) return {persistent(Y{}, Y{}, Y{}), persist_waves<true>()};
    if (s.grid) return s.persist ? Kernel{persistent(Y{}, Y{}, N{}), kPWaves} : Kernel{one_shot(N{}, N{}, Y{}), kWaves};
  }
  if (s.persist) return {s.lds_objs ? persistent(Y{}, N{}, N{}) : persistent(N{}, N{}, N{}), kPWaves};
  return {s.lds_objs ? one_shot(Y{}, Y{}, N{}) : s.lds_nodes ? one_shot(Y{}, N{}, N{}) : one_shot(N{}, N{}, N{}), kWaves};
}

Kernel kernel_of(Form form, int tri, const Shape &s) {
  using Fn = Kernel (*)(const Shape &);
#define RTMI_NW_FAMILIES(F) {kernel_ft<F, 0>, kernel_ft<F, 1>, kernel_ft<F, 2>, kernel_ft<F, 3>, kernel_ft<F, 4>, kernel_ft<F, 5>}
  static constexpr Fn table[kForms][kFamilies] = {RTMI_NW_FAMILIES(kOneShot), RTMI_NW_FAMILIES(kChunked), RTMI_NW_FAMILIES(kAdapt)};
#undef RTMI_NW_FAMILIES
  return table[form][tri](s);
}

// resident blocks per CU of a persistent kernel that stages nothing yet (rt_nw_ctx_create)
int blocks_per_cu(const Shape &s, int *per_cu) {
  const Kernel k = kernel_of(kChunked, 0, s);
  *per_cu = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, k.fn, 64 * k.waves, 0));
  return RT_OK;
}

}  // namespace

RTMI_EXPORT int rt_nw_ctx_create(int32_t device, rt_nw_ctx **out) {
  if (!out) return set_error(RT_EINVAL, "null out");
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return set_error(RT_ENODEVICE, "no HIP device visible");
  if (device < 0 || device >= count) return set_error(RT_ENODEVICE, "device %d out of range [0,%d)", device, count);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return set_error(RT_ENODEVICE, "device %d is %s; librtmi is built for gfx950 only", device, prop.gcnArchName);
  Guard g(device);
  auto ctx = std::make_unique<rt_nw_ctx>();
  ctx->device = device;
  HIP_TRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&ctx->last_done, hipEventDisableTiming));
  if (int rc = alloc_copy<unsigned long long>(&ctx->segments, nullptr, 1)) return rc;
  HIP_TRY(hipMemset(ctx->segments, 0, sizeof(unsigned long long)));
  if (int rc = alloc_copy<unsigned>(&ctx->counter, nullptr, 1)) return rc;
  {  // what stays resident of the persistent kernels (VGPR-limited: one 16-wave block per CU): the BVH shape that
     // stages the nodes alone, the general grid shape and its spheres-only instantiation
    Shape s;
    s.persist = s.lds_nodes = true;
    int per_cu = 0;
    if (int rc = blocks_per_cu(s, &per_cu)) return rc;
    ctx->persist_blocks = per_cu * prop.multiProcessorCount;
    s.grid = true;
    s.lds_nodes = false;
    if (int rc = blocks_per_cu(s, &per_cu)) return rc;
    ctx->persist_blocks_grid = per_cu * prop.multiProcessorCount;
    s.simple = true;
    if (int rc = blocks_per_cu(s, &per_cu)) return rc;
    ctx->persist_blocks_simple = per_cu * prop.multiProcessorCount;
    ctx->cus = prop.multiProcessorCount;
  }
  *out = ctx.release();
  return RT_OK;
}

RTMI_EXPORT int rt_nw_ctx_destroy(rt_nw_ctx *ctx) {
  delete ctx;  // (~rt_nw_ctx)
  return RT_OK;
}

RTMI_EXPORT int rt_nw_ctx_set_scene(rt_nw_ctx *ctx, rt_nw_scene *s) {
  if (!ctx || !s) return set_error(RT_EINVAL, "rt_nw_ctx_set_scene: null");
  DeviceScene ds;
  if (int rc = build_device_scene(s, ds)) return rc;
  // every index the kernel follows is checked here, once
  const int32_t nt = int32_t(ds.tex.size()), nm = int32_t(ds.mat.size()), ni = int32_t(ds.inst.size());
  const int32_t np = int32_t(ds.perlin_perm.size() / (3 * kPerlinN)), nim = int32_t(ds.image.size());
  const bool two_level = !ds.place_mesh.empty();
  int32_t n_moving = 0, n_affine = 0;
  for (const Obj &o : ds.obj) {
    if (o.mat < 0 || o.mat >= nm || o.inst >= ni || o.kind < kSphere ||
        (o.kind > kBox && o.kind != kTriangle && !(two_level && o.kind == kInstance)) || o.aux < 0 ||
        o.aux > (o.kind == kInstance ? 3 : int32_t(ds.med.size())))
      return set_error(RT_EINVAL, "rt_nw: object with bad material/instance/kind");
    if (o.kind != kInstance) continue;
    // a placement's motion words (rtmi_nw_types.h kInstance): all zero, or a
    // moving placement's — an Inst with the translation flag, o1 and two times
    // the walk can divide by
    if (o.aux == 0) {
      if (o.g1[1] != 0.f || o.g1[2] != 0.f || o.g1[3] != 0.f || o.g2[0] != 0.f || o.g2[1] != 0.f)
        return set_error(RT_EINVAL, "rt_nw: static placement with motion words");
      continue;
    }
    if (o.aux & 2) {
      // an affine placement's words (rtmi_nw_types.h AffInst): its row pair in
      // range, a finite matrix and offset, the affine flag
      ++n_affine;
      if (o.inst < 0 || o.inst + 1 >= ni) return set_error(RT_EINVAL, "rt_nw: affine placement with its rows out of range");
      AffInst ai;
      std::memcpy(&ai, &ds.inst[size_t(o.inst)], sizeof ai);
      bool ok = ai.flags == 4;
      for (float v : ai.m) ok = ok && std::isfinite(v);
      for (float v : ai.off) ok = ok && std::isfinite(v);
      if (!ok) return set_error(RT_EINVAL, "rt_nw: bad affine placement rows");
      if (o.aux == 2) {
        if (o.g1[1] != 0.f || o.g1[2] != 0.f || o.g1[3] != 0.f || o.g2[0] != 0.f || o.g2[1] != 0.f)
          return set_error(RT_EINVAL, "rt_nw: static placement with motion words");
        continue;
      }
      ++n_moving;
      if (!std::isfinite(o.g1[1]) || !std::isfinite(o.g1[2]) || !std::isfinite(o.g1[3]) || !std::isfinite(o.g2[0]) ||
          !std::isfinite(o.g2[1]) || o.g2[0] == o.g2[1])
        return set_error(RT_EINVAL, "rt_nw: bad motion in a placement record");
      continue;
    }
    ++n_moving;
    if (o.inst < 0 || !(ds.inst[size_t(o.inst)].flags & 2) || !std::isfinite(o.g1[1]) || !std::isfinite(o.g1[2]) ||
        !std::isfinite(o.g1[3]) || !std::isfinite(o.g2[0]) || !std::isfinite(o.g2[1]) || o.g2[0] == o.g2[1])
      return set_error(RT_EINVAL, "rt_nw: bad motion in a placement record");
  }
  if (n_moving != ds.n_moving) return set_error(RT_EINVAL, "rt_nw: moving placement records do not match the count");
  if (n_affine != ds.n_affine) return set_error(RT_EINVAL, "rt_nw: affine placement records do not match the count");
  // shared meshes: every link the two-level walk follows (rtmi_nw_path.h hit_world_nw_inst)
  const size_t npool = ds.pool.size(), nbot = ds.bnodes.size();
  if (!two_level && (npool || nbot || !ds.mesh.empty())) return set_error(RT_EINVAL, "rt_nw: shared pool without a placement");
  if (two_level) {
    if (ds.pool_j.size() != npool || ds.place_slot.size() != ds.place_mesh.size())
      return set_error(RT_EINVAL, "rt_nw: shared mesh tables do not match");
    for (const Obj &o : ds.pool)
      if (o.kind != kTriangle || o.mat < 0 || o.mat >= nm || o.inst != -1 || o.aux != 0)
        return set_error(RT_EINVAL, "rt_nw: bad record in a shared pool");
    for (const DeviceScene::SharedMesh &M : ds.mesh) {
      if (M.node0 < 0 || M.n_nodes < 0 || size_t(M.node0) + size_t(M.n_nodes) > nbot || M.pool0 < 0 || M.n_pool < 0 ||
          size_t(M.pool0) + size_t(M.n_pool) > npool || (M.n_pool > 0) != (M.n_nodes > 0))
        return set_error(RT_EINVAL, "rt_nw: shared mesh out of range");
      for (int32_t i = M.node0; i < M.node0 + M.n_nodes; ++i) {
        const Node &nd = ds.bnodes[size_t(i)];
        const int32_t first = nd.leaf >> 4, cnt = nd.leaf & 15;
        if (nd.skip <= i || nd.skip > M.node0 + M.n_nodes ||
            (nd.leaf >= 0 && (cnt < 1 || first < M.pool0 || first + cnt > M.pool0 + M.n_pool)))
          return set_error(RT_EINVAL, "rt_nw: bottom-level link out of its mesh");
      }
      for (int32_t q = M.pool0; q < M.pool0 + M.n_pool; ++q)
        if (ds.pool_j[size_t(q)] < 0 || ds.pool_j[size_t(q)] >= M.n_tris) return set_error(RT_EINVAL, "rt_nw: bad triangle number in a shared pool");
    }
    size_t n_records = 0;
    for (size_t k = 0; k < ds.obj.size(); ++k) n_records += ds.obj[k].kind == kInstance;
    size_t n_slots = 0;
    for (size_t p = 0; p < ds.place_mesh.size(); ++p) {
      const int32_t k = ds.place_slot[p], mi = ds.place_mesh[p];
      if (mi < 0 || size_t(mi) >= ds.mesh.size()) return set_error(RT_EINVAL, "rt_nw: placement of an unknown mesh");
      if (k < 0) continue;  // (a mesh without a triangle that can be hit)
      ++n_slots;
      const DeviceScene::SharedMesh &M = ds.mesh[size_t(mi)];
      int32_t w[4], np;
      if (size_t(k) >= ds.obj.size() || ds.obj[size_t(k)].kind != kInstance) return set_error(RT_EINVAL, "rt_nw: placement without its record");
      std::memcpy(w, ds.obj[size_t(k)].g0, sizeof w);
      std::memcpy(&np, &ds.obj[size_t(k)].g1[0], 4);
      if (w[0] != M.node0 || w[1] != M.node0 + M.n_nodes || w[2] != M.pool0 || np != M.n_pool || M.n_nodes < 1 || w[3] < 0 ||
          int64_t(w[3]) + M.n_tris > (int64_t(1) << 27))
        return set_error(RT_EINVAL, "rt_nw: placement record does not match its mesh");
    }
    if (n_slots != n_records) return set_error(RT_EINVAL, "rt_nw: placement records do not match the placements");
    for (const Node &nd : ds.nodes) {  // a placement is alone in its leaf
      if (nd.leaf < 0) continue;
      const int32_t first = nd.leaf >> 4, cnt = nd.leaf & 15;
      if (first < 0 || size_t(first) + size_t(cnt) > ds.obj.size()) return set_error(RT_EINVAL, "rt_nw: leaf out of range");
      for (int32_t k = first; k < first + cnt; ++k)
        if (ds.obj[size_t(k)].kind == kInstance && cnt != 1) return set_error(RT_EINVAL, "rt_nw: placement shares a leaf");
    }
  }
  for (const Obj &o : ds.med) {
    const int bk = o.aux & 255, ns = o.aux >> 8;
    if (o.mat < 0 || o.mat >= nm || o.inst >= ni || o.kind != kMedium || (bk != kSphere && bk != kMovingSphere && bk != kBox) ||
        ns < 1 || ns > 8)
      return set_error(RT_EINVAL, "rt_nw: bad medium record");
  }
  for (const Mat &m : ds.mat)
    if (m.kind != kDielectric && (m.tex < 0 || m.tex >= nt)) return set_error(RT_EINVAL, "rt_nw: material with bad texture");
  for (const Tex &t : ds.tex) {
    if (t.kind == kChecker && (t.a < 0 || t.a >= nt || t.b < 0 || t.b >= nt)) return set_error(RT_EINVAL, "rt_nw: bad checker");
    if (t.kind == kNoise && (t.a < 0 || t.a >= np)) return set_error(RT_EINVAL, "rt_nw: bad perlin index");
    if (t.kind == kImage && (t.a < 0 || t.a >= nim)) return set_error(RT_EINVAL, "rt_nw: bad image index");
  }
  // nodes as lo[] = {bmin, skip} and hi[] = {bmax, leaf} (two independent loads)
  // ... then the bottom-level nodes of shared meshes, as {lo, hi} pairs
  std::vector<float4> split(2 * ds.nodes.size() + 2 * nbot);
  for (size_t i = 0; i < ds.nodes.size(); ++i) {
    const Node &nd = ds.nodes[i];
    float sk, lf;
    std::memcpy(&sk, &nd.skip, 4);
    std::memcpy(&lf, &nd.leaf, 4);
    split[i] = make_float4(nd.bmin[0], nd.bmin[1], nd.bmin[2], sk);
    split[ds.nodes.size() + i] = make_float4(nd.bmax[0], nd.bmax[1], nd.bmax[2], lf);
  }
  for (size_t i = 0; i < nbot; ++i) {
    const Node &nd = ds.bnodes[i];
    float sk, lf;
    std::memcpy(&sk, &nd.skip, 4);
    std::memcpy(&lf, &nd.leaf, 4);
    split[2 * ds.nodes.size() + 2 * i] = make_float4(nd.bmin[0], nd.bmin[1], nd.bmin[2], sk);
    split[2 * ds.nodes.size() + 2 * i + 1] = make_float4(nd.bmax[0], nd.bmax[1], nd.bmax[2], lf);
  }
  // attribute records: the locator holds one entry per object, -1 or a record of a triangle
  const size_t nattr = ds.obj_attr.empty() ? 0 : ds.attr.size();
  if (!ds.obj_attr.empty() && (ds.obj_attr.size() != ds.obj.size() || nattr == 0))
    return set_error(RT_EINVAL, "rt_nw: attribute locator does not match the objects");
  for (size_t i = 0; i < ds.obj_attr.size(); ++i)
    if (ds.obj_attr[i] < -1 || ds.obj_attr[i] >= int32_t(nattr) || (ds.obj_attr[i] >= 0 && ds.obj[i].kind != kTriangle))
      return set_error(RT_EINVAL, "rt_nw: attribute record index out of range");
  if (ds.pool_attr.size() != (nattr ? npool : 0)) return set_error(RT_EINVAL, "rt_nw: attribute locator does not match the shared pool");
  for (int32_t a : ds.pool_attr)
    if (a < -1 || a >= int32_t(nattr)) return set_error(RT_EINVAL, "rt_nw: attribute record index out of range");
  // the records follow the objects in one allocation and the locator follows
  // the insertion indices (rtmi_nw_path.h attr_view_of): 64 B records behind
  // 48 B ones, so the tail is sized in DevObj units
  // With placements (rtmi_nw_path.h pool_view_of): the pool between the
  // objects and the records; behind the insertion indices {pool slots,
  // attribute records}, the pool's triangle numbers, then the locator over
  // objects and pool slots.
  const size_t nrec = ds.obj.size() + npool;
  std::vector<DevObj> dobj(nrec + (nattr * sizeof(TriAttr) + sizeof(DevObj) - 1) / sizeof(DevObj));
  if (nattr) std::memcpy(static_cast<void *>(dobj.data() + nrec), ds.attr.data(), nattr * sizeof(TriAttr));
  std::vector<int32_t> dobj_id = ds.obj_id;
  if (two_level) {
    dobj_id.push_back(int32_t(npool));
    dobj_id.push_back(int32_t(nattr));
    dobj_id.insert(dobj_id.end(), ds.pool_j.begin(), ds.pool_j.end());
  }
  if (nattr) dobj_id.insert(dobj_id.end(), ds.obj_attr.begin(), ds.obj_attr.end());
  if (nattr) dobj_id.insert(dobj_id.end(), ds.pool_attr.begin(), ds.pool_attr.end());
  for (size_t i = 0; i < nrec; ++i) {
    const Obj &o = i < ds.obj.size() ? ds.obj[i] : ds.pool[i - ds.obj.size()];
    DevObj &q = dobj[i];
    for (int c = 0; c < 4; ++c) {
      q.g0[c] = o.g0[c];
      q.g1[c] = o.g1[c];
    }
    q.ka = o.kind | (o.aux << 8);
    q.mat = o.mat;
    if (o.kind == kInstance) std::memcpy(&q.mat, &o.g2[1], 4);  // time0 of a moving placement (else zero bits)
    q.t1 = o.g2[0];
    q.inst = o.inst;
  }
  std::vector<float4> pv(ds.perlin_vec.size() / 4);
  std::memcpy(pv.data(), ds.perlin_vec.data(), pv.size() * sizeof(float4));
  if (ds.grid_ok) {  // (checked before any device buffer is replaced)
    for (uint16_t r : ds.grid_refs)
      if (r >= ds.obj.size()) return set_error(RT_EINVAL, "rt_nw: grid reference out of range");
    for (int32_t b : ds.grid_big)
      if (b < 0 || size_t(b) >= ds.obj.size()) return set_error(RT_EINVAL, "rt_nw: brute-force index out of range");
  }
  Guard g(ctx->device);
  // the context's structures are replaced below: until that completes, no
  // render may use a mix of old counts and new buffers
  ctx->nobj = ctx->nmed = ctx->nnodes = ctx->nattr = ctx->npool = ctx->nbot = 0;
  ctx->grid_ok = false;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  int rc;
  if ((rc = alloc_copy(&ctx->obj, dobj.data(), dobj.size())) ||
      (rc = alloc_copy(&ctx->med, ds.med.data(), ds.med.size())) ||
      (rc = alloc_copy(&ctx->med_id, ds.med_id.data(), ds.med_id.size())) ||
      (rc = alloc_copy(&ctx->obj_id, dobj_id.data(), dobj_id.size())) ||
      (rc = alloc_copy(&ctx->inst, ds.inst.data(), ds.inst.size())) ||
      (rc = alloc_copy(&ctx->mat, ds.mat.data(), ds.mat.size())) ||
      (rc = alloc_copy(&ctx->tex, ds.tex.data(), ds.tex.size())) || (rc = alloc_copy(&ctx->pvec, pv.data(), pv.size())) ||
      (rc = alloc_copy(&ctx->pperm, ds.perlin_perm.data(), ds.perlin_perm.size())) ||
      (rc = alloc_copy(&ctx->img, ds.image_px.data(), ds.image_px.size())) ||
      (rc = alloc_copy(&ctx->imgd, ds.image.data(), ds.image.size())) ||
      (rc = alloc_copy(&ctx->nodes, split.data(), split.size())))
    return rc;
  if (ds.grid_ok) {
    if ((rc = alloc_copy(&ctx->grid_cells, ds.grid_cell_start.data(), ds.grid_cell_start.size())) ||
        (rc = alloc_copy(&ctx->grid_refs, ds.grid_refs.data(), ds.grid_refs.size())) ||
        (rc = alloc_copy(&ctx->grid_big, ds.grid_big.data(), ds.grid_big.size())))
      return rc;
    NwGridDesc &G = ctx->grid;
    for (int a = 0; a < 3; ++a) {
      G.g0[a] = ds.grid_g0[a];
      G.h[a] = ds.grid_h[a];
      G.inv_h[a] = ds.grid_inv_h[a];
      G.g1[a] = ds.grid_g1[a];
      G.n[a] = ds.grid_n[a];
    }
    G.ncells = int32_t(ds.grid_cell_start.size()) - 1;
    G.nrefs = int32_t(ds.grid_refs.size());
    G.cell_start = ctx->grid_cells;
    G.refs = ctx->grid_refs;
    ctx->nbig = int32_t(ds.grid_big.size());
    ctx->grid_max_cell = ds.grid_max_cell;
  } else {
    ctx->grid = NwGridDesc{};
    ctx->nbig = 0;
    ctx->grid_max_cell = 0;
  }
  ctx->grid_ok = ds.grid_ok;
  ctx->nobj = int32_t(ds.obj.size());
  ctx->nmed = int32_t(ds.med.size());
  ctx->nnodes = int32_t(ds.nodes.size());
  ctx->ninst = ni;
  ctx->nmat = nm;
  ctx->ntex = nt;
  for (int c = 0; c < 3; ++c) ctx->bg[c] = ds.background[c];
  ctx->has_media = ds.has_media ? 1 : 0;
  ctx->has_tri = 0;
  for (const Obj &o : ds.obj) ctx->has_tri |= o.kind == kTriangle ? 1 : 0;
  ctx->nattr = int32_t(nattr);
  if (nattr) ctx->has_tri = 2;
  if (two_level) ctx->has_tri = ds.n_affine > 0 ? 5 : ds.n_moving > 0 ? 4 : 3;
  ctx->npool = int32_t(npool);
  ctx->nbot = int32_t(nbot);
  bool simple = ds.med.empty();
  for (const Obj &o : ds.obj) simple = simple && o.inst < 0 && (o.kind == kSphere || o.kind == kMovingSphere);
  for (const Tex &t : ds.tex)
    simple = simple && (t.kind == kSolid || (t.kind == kChecker && ds.tex[size_t(t.a)].kind == kSolid &&
                                             ds.tex[size_t(t.b)].kind == kSolid));
  ctx->simple = simple;
  return RT_OK;
}

RTMI_EXPORT int rt_nw_ctx_info(rt_nw_ctx *ctx, int32_t *n_prims, int32_t *n_nodes) {
  if (!ctx) return set_error(RT_EINVAL, "null ctx");
  if (n_prims) *n_prims = ctx->nobj + ctx->nmed;
  if (n_nodes) *n_nodes = ctx->nnodes;
  return RT_OK;
}

namespace {
// The structure a render uses (RT_NW_ACCEL_BVH or _GRID) and whether its
// grid fits the LDS of the persistent / grid kernel shapes.
constexpr int32_t kNwGridMaxCell = 24;  // AUTO: a grid with a fuller cell renders with the BVH
size_t grid_bytes(const rt_nw_ctx *c) {
  return nw_grid_lds_bytes(c->nobj, c->grid.ncells, c->grid.nrefs, c->nbig);
}
// a grid renders with the persistent kernel
bool grid_persists(const rt_nw_ctx *c) { return RTMI_NW_PERSIST && c->persist_ok && c->persist_blocks_grid > 0; }
int32_t accel_used(const rt_nw_ctx *c) {
  // the grid is staged whole: by the persistent kernel (one block per CU)
  // when it runs, else by the grid kernel's per-block budget; a grid that
  // fits neither renders with the BVH
  const bool fits = c->grid_ok && grid_bytes(c) <= (grid_persists(c) ? kPLdsBudget : kLdsBudget);
  if (c->accel == RT_NW_ACCEL_GRID) return fits ? RT_NW_ACCEL_GRID : RT_NW_ACCEL_BVH;
  if (c->accel == RT_NW_ACCEL_BVH) return RT_NW_ACCEL_BVH;
  return fits && c->grid_max_cell <= kNwGridMaxCell ? RT_NW_ACCEL_GRID : RT_NW_ACCEL_BVH;
}
}  // namespace

RTMI_EXPORT int rt_nw_ctx_set_accel(rt_nw_ctx *ctx, int32_t accel) {
  if (!ctx) return set_error(RT_EINVAL, "null ctx");
  if (accel != RT_NW_ACCEL_AUTO && accel != RT_NW_ACCEL_BVH && accel != RT_NW_ACCEL_GRID)
    return set_error(RT_EINVAL, "rt_nw_ctx_set_accel: unknown structure %d", accel);
  ctx->accel = accel;
  return RT_OK;
}

RTMI_EXPORT int rt_nw_ctx_accel_info(rt_nw_ctx *ctx, int32_t *accel, int32_t *dims3, int32_t *max_cell, int32_t *n_big) {
  if (!ctx) return set_error(RT_EINVAL, "null ctx");
  if (accel) *accel = accel_used(ctx);
  if (dims3)
    for (int a = 0; a < 3; ++a) dims3[a] = ctx->grid_ok ? ctx->grid.n[a] : 0;
  if (max_cell) *max_cell = ctx->grid_ok ? ctx->grid_max_cell : 0;
  if (n_big) *n_big = ctx->grid_ok ? ctx->nbig : 0;
  return RT_OK;
}

namespace {
// rt_nw_render_rows, and with pass_accum set a progressive pass (rt_nw_render_pass): samples s_base + [0, spp)
// of the rows are added to that fixed-point accumulator ([nrows][W][3], zeroed by rt_nw_accum_reset) by the
// CHUNKED instantiation of the same kernel shape; nothing is cleared, no float is written and dev_strip is
// not read.  `who` names the entry point in error messages.
int check_rows_args(rt_nw_ctx *ctx, const rt_nw_camera *cam, int32_t W, int32_t H, int32_t spp, int32_t max_depth,
                    int32_t row0, int32_t row_step, int32_t nrows, int32_t s_base, bool pass, const char *who) {
  if (!ctx || !cam) return set_error(RT_EINVAL, "%s: null argument", who);
  if (ctx->nobj + ctx->nmed <= 0) return set_error(RT_EINVAL, "no scene uploaded (rt_nw_ctx_set_scene)");
  if (W < 1 || H < 1 || spp < 1 || (!pass && spp >= (1 << 24)) || max_depth < 1 || max_depth >= (1 << 24) ||
      int64_t(W) * H >= (int64_t(1) << 40))
    return set_error(RT_EINVAL, "%s: bad size (W, H, spp >= 1, spp < 2^24, 1 <= max_depth < 2^24)", who);
  if (nrows < 1 || row_step < 1 || row0 < 0 || row0 >= H) return set_error(RT_EINVAL, "%s: bad row set", who);
  if (!(cam->time0 >= 0.0 && cam->time1 <= 1.0 && cam->time0 <= cam->time1))
    return set_error(RT_EINVAL, "%s: shutter must lie in [0, 1]", who);
  // a pass's samples keep inside the RNG key's 24 bits (checked by rt_nw_render_pass)
  if (s_base < 0 || int64_t(s_base) + spp > (int64_t(1) << 24)) return set_error(RT_EINVAL, "%s: bad sample range", who);
  return RT_OK;
}

// The shape of a launch of the context's scene, plain or adaptive.  The adaptive kernels' static LDS is larger, so
// they have staging budgets of their own, and a grid that fits the plain kernels' budget but not theirs is walked
// as a BVH by an adaptive pass (the same image).
int shape_of(const rt_nw_ctx *ctx, bool adapt, Shape &s) {
  const size_t p_budget = adapt ? kPLdsBudgetA : kPLdsBudget, p_two_budget = adapt ? kPTwoBlockBudgetA : kPTwoBlockBudget,
               g_budget = adapt ? kLdsBudgetA : kLdsBudget;
  const size_t node_bytes = size_t(ctx->nnodes) * 32, obj_bytes = size_t(ctx->nobj) * (sizeof(DevObj) + 4);
  s = Shape{};
  s.grid = accel_used(ctx) == RT_NW_ACCEL_GRID && (!adapt || grid_bytes(ctx) <= (grid_persists(ctx) ? p_budget : g_budget));
  // persistent when the grid, or the nodes, fit one CU's LDS budget; else one wave per work item
  s.persist = RTMI_NW_PERSIST && ctx->persist_ok && (s.grid ? ctx->persist_blocks_grid > 0 : ctx->persist_blocks > 0) &&
              (s.grid || (ctx->nnodes > 0 && node_bytes <= p_budget));
  if (s.grid) {
    s.lds = grid_bytes(ctx);
    if (!s.persist && s.lds > g_budget) return set_error(RT_EINVAL, "rt_nw: grid does not fit the grid kernel's LDS");
    if (ctx->has_tri >= 3) return set_error(RT_EINVAL, "rt_nw: a scene with placements has no grid");
    s.simple = s.persist && ctx->simple && ctx->simple_ok && ctx->persist_blocks_simple > 0;
    return RT_OK;
  }
  if (s.persist) {
    // objects staged beside the nodes only when two blocks still fit a CU (or
    // when one block per CU is all the nodes allow anyway)
    // (the two-level kernels below 8 waves per SIMD run one block per CU whatever they stage)
    const bool one_block = (ctx->has_tri == 3 && RTMI_NW_INST_PER_EU < 8) || (ctx->has_tri == 4 && RTMI_NW_MOVE_PER_EU < 8) ||
                           (ctx->has_tri == 5 && RTMI_NW_AFFINE_PER_EU < 8);
    s.lds_nodes = true;
    s.lds_objs = RTMI_NW_LDS_OBJS && (node_bytes + obj_bytes <= p_two_budget ||
                                      ((one_block || node_bytes > p_two_budget) && node_bytes + obj_bytes <= p_budget));
  } else {  // per block: the nodes when they fit, then the objects too
    s.lds_nodes = ctx->nnodes > 0 && node_bytes <= g_budget;
    s.lds_objs = RTMI_NW_LDS_OBJS && s.lds_nodes && node_bytes + obj_bytes <= g_budget;
  }
  s.lds = s.lds_nodes ? node_bytes + (s.lds_objs ? obj_bytes : 0) : 0;
  return RT_OK;
}

// The context's buffers (accumulators, counters, scratch) are shared by everything it launches: work on another
// stream first waits for the end of the last one ...
int take_turn(rt_nw_ctx *ctx, hipStream_t st) {
  if (ctx->last_stream && ctx->last_stream != st) HIP_TRY(hipStreamWaitEvent(st, ctx->last_done, 0));
  ctx->last_stream = st;
  return RT_OK;
}
// ... and records its own end, whatever path returns
struct MarkDone {
  rt_nw_ctx *c;
  hipStream_t s;
  ~MarkDone() { (void)hipEventRecord(c->last_done, s); }
};

// With adapt set (rt_nw_adapt_pass): pass_accum is the adaptive accumulator's sums, the work items cover the listed
// tiles only, each active pixel p takes the samples n[p] + [0, spp), and the ADAPT twin of the same shape runs.
struct AdaptLaunch {
  AdaptArgs dev;    // the uploaded list and the accumulator's n and m2
  int32_t n_tiles;  // active tiles
};

int render_rows_impl(rt_nw_ctx *ctx, const rt_nw_camera *cam, int32_t W, int32_t H, int32_t spp, int32_t max_depth,
                     uint64_t seed, int32_t row0, int32_t row_step, int32_t nrows, float *dev_strip, void *stream,
                     int32_t s_base, unsigned long long *pass_accum, const char *who, const AdaptLaunch *adapt = nullptr) {
  if (int rc = check_rows_args(ctx, cam, W, H, spp, max_depth, row0, row_step, nrows, s_base, pass_accum != nullptr, who)) return rc;
  if (!dev_strip && !pass_accum) return set_error(RT_EINVAL, "%s: null argument", who);
  const int32_t valid = std::min<int64_t>(nrows, (int64_t(H) - 1 - row0) / row_step + 1);
  Guard g(ctx->device);
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  Args a = camera_args(cam, W, H, max_depth, seed);
  a.s_end = s_base + spp;
  a.s_base = s_base;
  a.row0 = row0;
  a.row_step = row_step;
  a.nrows_valid = valid;
  a.tiles_x = (W + 7) / 8;
  a.tiles = adapt ? adapt->n_tiles : a.tiles_x * ((valid + 7) / 8);
  Shape sh;
  if (int rc = shape_of(ctx, adapt != nullptr, sh)) return rc;
  // The kernel that is asked about (its static LDS, how many of its blocks stay resident) is the accumulating
  // instantiation even when the float-writing one launches below: the two of a shape have equal VGPR, SGPR and
  // LDS figures (profiles/adaptive/kernel_resources.txt), and the answer is needed before the launch knows
  // whether one work item per tile is enough.
  const Form asked = adapt ? kAdapt : kChunked;
  const Kernel ask = kernel_of(asked, ctx->has_tri, sh);
  if (int rc = take_turn(ctx, st)) return rc;
  MarkDone mark_done{ctx, st};
  if (valid < nrows && !pass_accum)  // rows past H: zero (a pass leaves them as rt_nw_accum_reset zeroed them)
    HIP_TRY(hipMemsetAsync(dev_strip + size_t(valid) * W * 3, 0, size_t(nrows - valid) * W * 3 * sizeof(float), st));
  HIP_TRY(hipMemsetAsync(ctx->segments, 0, sizeof(unsigned long long), st));
  {
    hipFuncAttributes fa;
    HIP_TRY(hipFuncGetAttributes(&fa, ask.fn));
    if (fa.sharedSizeBytes + sh.lds > kCuLds)
      return set_error(RT_EINVAL, "rt_nw: %zu B staged + %zu B static LDS exceed a CU's %zu B", sh.lds,
                       size_t(fa.sharedSizeBytes), kCuLds);
  }
  // samples per work item (same image for any size; RTMI_NW_CHUNK overrides,
  // for A/B).  Persistent kernel: ~80 items per resident wave, 4..32 samples:
  // the final scene (fog, lights: long and uneven paths) at 256 spp runs 329
  // ms with 8, 433 with 32; at 1024 spp 1215 ms with 24, 1205 with 32, 1308
  // with 8 — the item count, not the size, sets its tail
  // (profiles/r01/session6/nw_chunk.txt).  Grid kernel: 32.
  int64_t chunk = 32;
  int32_t resident = 0;  // persistent: the blocks that stay resident with the staged bytes
  if (sh.persist) {
    const auto key = std::make_pair(ask.fn, sh.lds);
    auto it = std::find_if(ctx->occupancy.begin(), ctx->occupancy.end(), [&](const auto &e) { return e.first == key; });
    if (it == ctx->occupancy.end()) {
      int per_cu = 0;
      HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, ask.fn, 64 * ask.waves, sh.lds));
      ctx->occupancy.push_back({key, std::max(1, per_cu) * ctx->cus});
      it = ctx->occupancy.end() - 1;
    }
    resident = it->second;
    chunk = std::min<int64_t>(32, std::max<int64_t>(4, int64_t(a.tiles) * spp / (80 * int64_t(resident) * ask.waves)));
  }
  // (at most 65535 samples per item: job indices stay below 2^22, where the
  // kernels' reciprocal-multiply job decode is exact)
  a.chunk = std::min<int64_t>({spp, ctx->env_chunk > 0 ? ctx->env_chunk : chunk, 65535});
  a.nch = (spp + a.chunk - 1) / a.chunk;
  if (int64_t(a.tiles) * a.nch >= (int64_t(1) << 31) - kWaves) return set_error(RT_EINVAL, "render too large");
  a.n_items = a.tiles * a.nch;
  const unsigned blocks = unsigned(sh.persist ? std::min<int64_t>(resident, (a.n_items + ask.waves - 1) / ask.waves)
                                              : (a.n_items + kWaves - 1) / kWaves);
  if (sh.persist) HIP_TRY(hipMemsetAsync(ctx->counter, 0, sizeof(unsigned), st));
  ctx->last_kernel[0] = sh.persist ? 1 : 0;
  ctx->last_kernel[1] = sh.grid ? 1 : 0;
  ctx->last_kernel[2] = sh.simple ? 1 : 0;
  ctx->last_kernel[3] = a.chunk;
  ctx->last_staging[0] = sh.lds_nodes ? 1 : 0;
  ctx->last_staging[1] = sh.grid || sh.lds_objs ? 1 : 0;
  // A pass adds into its own accumulator, whatever nch is: no memset, no finalize (rt_nw_accum_resolve).  A render
  // of several items per tile adds into ctx->accum, the per-render scratch; one item per tile writes the floats.
  unsigned long long *acc_buf = pass_accum;
  const size_t nv = size_t(valid) * W * 3;
  const bool scratch = !pass_accum && a.nch > 1;
  if (scratch) {
    if (nv > ctx->accum_cap) {
      HIP_TRY(hipStreamSynchronize(st));
      if (int rc = alloc_copy<unsigned long long>(&ctx->accum, nullptr, nv)) return rc;
      ctx->accum_cap = nv;
    }
    HIP_TRY(hipMemsetAsync(ctx->accum, 0, nv * sizeof(unsigned long long), st));
    acc_buf = ctx->accum;
  }
  const Kernel k = kernel_of(pass_accum || scratch ? asked : kOneShot, ctx->has_tri, sh);
  View v = view_of(ctx);
  AdaptArgs ad = adapt ? adapt->dev : AdaptArgs{};
  // View, Args, [AdaptArgs,] accum, [out,] segments [, counter]
  void *args[6] = {&v, &a, adapt ? (void *)&ad : (void *)&acc_buf, adapt ? (void *)&acc_buf : (void *)&dev_strip, &ctx->segments,
                   &ctx->counter};
  HIP_TRY(hipLaunchKernel(k.fn, dim3(blocks), dim3(64 * k.waves), args, sh.lds, st));
  if (scratch) {
    hipLaunchKernelGGL(finalize_kernel, dim3(unsigned((nv + 255) / 256)), dim3(256), 0, st, ctx->accum, dev_strip, nv);
    HIP_TRY(hipGetLastError());
  }
  return RT_OK;
}
}  // namespace

RTMI_EXPORT int rt_nw_render_rows(rt_nw_ctx *ctx, const rt_nw_camera *cam, int32_t W, int32_t H, int32_t spp,
                                  int32_t max_depth, uint64_t seed, int32_t row0, int32_t row_step, int32_t nrows,
                                  float *dev_strip, void *stream) {
  if (!dev_strip) return set_error(RT_EINVAL, "rt_nw_render_rows: null argument");
  return render_rows_impl(ctx, cam, W, H, spp, max_depth, seed, row0, row_step, nrows, dev_strip, stream, 0, nullptr,
                          "rt_nw_render_rows");
}

RTMI_EXPORT int rt_nw_render(rt_nw_ctx *ctx, const rt_nw_camera *cam, int32_t W, int32_t H, int32_t spp,
                             int32_t max_depth, uint64_t seed, float *sum) {
  if (!ctx || !sum) return set_error(RT_EINVAL, "rt_nw_render: null argument");
  if (W < 1 || H < 1 || int64_t(W) * H >= (int64_t(1) << 40)) return set_error(RT_EINVAL, "rt_nw_render: bad size");
  Guard g(ctx->device);
  const size_t n = size_t(W) * size_t(H) * 3;
  if (n > ctx->scratch_cap) {
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (int rc = alloc_copy<float>(&ctx->scratch, nullptr, n)) return rc;
    ctx->scratch_cap = n;
  }
  if (int rc = rt_nw_render_rows(ctx, cam, W, H, spp, max_depth, seed, 0, 1, H, ctx->scratch, ctx->stream)) return rc;
  HIP_TRY(hipMemcpyAsync(sum, ctx->scratch, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return RT_OK;
}

// ---------------------------------------------------------------------------
// progressive passes (DESIGN.md §9 "Progressive passes"; as rtmi_device.hip's)
// ---------------------------------------------------------------------------
// The pass accumulator holds the fixed-point sums (2^-32, int64) of the passes
// so far.  A sample's contribution depends on (seed, pixel, sample index) alone
// and integer addition has no order, so any split of [0, spp) into passes gives
// the sums of one rt_nw_render of spp samples, bit for bit.
RTMI_EXPORT int rt_nw_accum_reset(rt_nw_ctx *ctx, int32_t W, int32_t nrows) {
  if (!ctx) return set_error(RT_EINVAL, "null ctx");
  if (W < 1 || nrows < 1 || int64_t(W) * nrows >= (int64_t(1) << 40))
    return set_error(RT_EINVAL, "rt_nw_accum_reset: bad size %dx%d", W, nrows);
  Guard g(ctx->device);
  const size_t n = size_t(W) * size_t(nrows) * 3;
  if (ctx->last_stream) HIP_TRY(hipStreamSynchronize(ctx->last_stream));  // no pass still adding
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (ctx->pass_cap < n) {
    ctx->pass_cap = 0;
    ctx->pass_W = ctx->pass_rows = ctx->pass_spp = 0;
    if (int rc = alloc_copy<unsigned long long>(&ctx->pass_accum, nullptr, n)) return rc;
    ctx->pass_cap = n;
  }
  ctx->pass_W = W;
  ctx->pass_rows = nrows;
  ctx->pass_spp = 0;
  HIP_TRY(hipMemsetAsync(ctx->pass_accum, 0, n * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return RT_OK;
}

RTMI_EXPORT int rt_nw_render_pass(rt_nw_ctx *ctx, const rt_nw_camera *cam, int32_t W, int32_t H, int32_t s_begin,
                                  int32_t s_count, int32_t max_depth, uint64_t seed, int32_t row0, int32_t row_step,
                                  int32_t nrows, void *stream) {
  if (!ctx || !cam) return set_error(RT_EINVAL, "rt_nw_render_pass: null argument");
  // (the RNG key gives a sample 24 bits; 2^24 samples of at most 64.0 stay below 2^62 in the accumulator)
  if (s_begin < 0 || s_count < 0 || int64_t(s_begin) + s_count > (int64_t(1) << 24))
    return set_error(RT_EINVAL, "rt_nw_render_pass: bad sample range [%d, +%d) (samples lie in [0, 2^24))", s_begin, s_count);
  if (!ctx->pass_accum || !ctx->pass_W || W != ctx->pass_W || nrows != ctx->pass_rows)
    return set_error(RT_EINVAL, "rt_nw_render_pass: accumulator is not %dx%d (call rt_nw_accum_reset)", W, nrows);
  if (size_t(W) * size_t(nrows) * 3 > ctx->pass_cap) return set_error(RT_EHIP, "internal: pass accumulator too small");
  if (s_count == 0)  // nothing to add: the arguments are still a render's
    return check_rows_args(ctx, cam, W, H, 1, max_depth, row0, row_step, nrows, s_begin == (1 << 24) ? 0 : s_begin, true, "rt_nw_render_pass");
  if (int rc = render_rows_impl(ctx, cam, W, H, s_count, max_depth, seed, row0, row_step, nrows, nullptr, stream, s_begin,
                                ctx->pass_accum, "rt_nw_render_pass"))
    return rc;
  ctx->pass_spp += s_count;
  return RT_OK;
}

RTMI_EXPORT int rt_nw_accum_resolve(rt_nw_ctx *ctx, float *dev_sum, float *host_sum, void *stream) {
  if (!ctx) return set_error(RT_EINVAL, "null ctx");
  if (!ctx->pass_accum || !ctx->pass_W) return set_error(RT_EINVAL, "rt_nw_accum_resolve: no accumulator (rt_nw_accum_reset)");
  if (!dev_sum && !host_sum) return set_error(RT_EINVAL, "rt_nw_accum_resolve: no output");
  Guard g(ctx->device);
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  const size_t n = size_t(ctx->pass_W) * size_t(ctx->pass_rows) * 3;
  float *out = dev_sum;
  if (!out) {  // through the context's float scratch, which renders share
    if (n > ctx->scratch_cap) {
      if (ctx->last_stream) HIP_TRY(hipStreamSynchronize(ctx->last_stream));
      HIP_TRY(hipStreamSynchronize(ctx->stream));
      ctx->scratch_cap = 0;
      if (int rc = alloc_copy<float>(&ctx->scratch, nullptr, n)) return rc;
      ctx->scratch_cap = n;
    }
    out = ctx->scratch;
  }
  // a resolve on another stream waits for the last pass (and, as it may write the shared scratch, it is
  // itself work the next render waits for)
  if (int rc = take_turn(ctx, st)) return rc;
  hipLaunchKernelGGL(finalize_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, st, ctx->pass_accum, out, n);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && host_sum) e = hipMemcpyAsync(host_sum, out, n * sizeof(float), hipMemcpyDeviceToHost, st);
  (void)hipEventRecord(ctx->last_done, st);
  if (e == hipSuccess && host_sum) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error(RT_EHIP, "rt_nw_accum_resolve: %s", hipGetErrorString(e));
  return RT_OK;
}

// Checkpoint / resume: the raw fixed-point accumulator (W * nrows * 3 int64) and the number of samples it holds.
RTMI_EXPORT int rt_nw_accum_export(rt_nw_ctx *ctx, int64_t *host, size_t n, int32_t *spp_done) {
  if (!ctx || !host) return set_error(RT_EINVAL, "rt_nw_accum_export: null argument");
  const size_t want = size_t(ctx->pass_W) * size_t(ctx->pass_rows) * 3;
  if (!ctx->pass_accum || !want || n != want)
    return set_error(RT_EINVAL, "rt_nw_accum_export: size %zu, accumulator %zu (rt_nw_accum_reset)", n, want);
  Guard g(ctx->device);
  HIP_TRY(hipStreamSynchronize(ctx->last_stream ? ctx->last_stream : ctx->stream));
  HIP_TRY(hipMemcpy(host, ctx->pass_accum, n * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (spp_done) *spp_done = ctx->pass_spp;
  return RT_OK;
}

RTMI_EXPORT int rt_nw_accum_import(rt_nw_ctx *ctx, const int64_t *host, size_t n, int32_t spp_done) {
  if (!ctx || !host) return set_error(RT_EINVAL, "rt_nw_accum_import: null argument");
  const size_t want = size_t(ctx->pass_W) * size_t(ctx->pass_rows) * 3;
  if (!ctx->pass_accum || !want || n != want)
    return set_error(RT_EINVAL, "rt_nw_accum_import: size %zu, accumulator %zu (call rt_nw_accum_reset)", n, want);
  if (spp_done < 0 || spp_done > (1 << 24)) return set_error(RT_EINVAL, "rt_nw_accum_import: sample count outside [0, 2^24]");
  Guard g(ctx->device);
  if (ctx->last_stream) HIP_TRY(hipStreamSynchronize(ctx->last_stream));
  HIP_TRY(hipMemcpy(ctx->pass_accum, host, n * sizeof(int64_t), hipMemcpyHostToDevice));
  ctx->pass_spp = spp_done;
  return RT_OK;
}

RTMI_EXPORT int rt_nw_accum_save(rt_nw_ctx *ctx, const char *path, rt_nw_scene *scene, const rt_nw_camera *cam, int32_t H,
                                 int32_t row0, int32_t row_step, int32_t max_depth, uint64_t seed) {
  if (!ctx || !path || !scene || !cam) return set_error(RT_EINVAL, "rt_nw_accum_save: null argument");
  if (!ctx->pass_accum || !ctx->pass_W) return set_error(RT_EINVAL, "rt_nw_accum_save: no accumulator (rt_nw_accum_reset)");
  CkptHeader h{};
  if (int rc = rt_nw_scene_hash(scene, &h.scene_hash)) return rc;
  const size_t n = size_t(ctx->pass_W) * size_t(ctx->pass_rows) * 3;
  std::vector<int64_t> raw(n);
  if (int rc = rt_nw_accum_export(ctx, raw.data(), n, &h.spp_done)) return rc;
  h.W = ctx->pass_W;
  h.H = H;
  h.row0 = row0;
  h.row_step = row_step;
  h.nrows = ctx->pass_rows;
  h.max_depth = max_depth;
  h.seed = seed;
  h.camera_hash = camera_hash(cam);
  return ckpt_write(path, h, raw.data());
}

RTMI_EXPORT int rt_nw_accum_load(rt_nw_ctx *ctx, const char *path, rt_nw_scene *scene, const rt_nw_camera *cam, int32_t W,
                                 int32_t H, int32_t row0, int32_t row_step, int32_t nrows, int32_t max_depth, uint64_t seed,
                                 int32_t *spp_done) {
  if (!ctx || !path || !scene || !cam || !spp_done) return set_error(RT_EINVAL, "rt_nw_accum_load: null argument");
  if (W < 1 || nrows < 1) return set_error(RT_EINVAL, "rt_nw_accum_load: bad size %dx%d", W, nrows);
  uint64_t sh = 0;
  if (int rc = rt_nw_scene_hash(scene, &sh)) return rc;
  CkptHeader h{};
  if (int rc = ckpt_read(path, h, nullptr)) return rc;
  if (h.W != W || h.H != H || h.row0 != row0 || h.row_step != row_step || h.nrows != nrows || h.max_depth != max_depth ||
      h.seed != seed || h.scene_hash != sh || h.camera_hash != camera_hash(cam))
    return set_error(RT_EINVAL, "rt_nw_accum_load: %s was made for another render (size, rows, depth, seed, scene or camera)",
                     path);
  if (h.spp_done < 0 || h.spp_done > (1 << 24)) return set_error(RT_EIO, "rt_nw_accum_load: %s holds a bad sample count", path);
  std::vector<int64_t> raw;
  if (int rc = ckpt_read(path, h, &raw)) return rc;  // (the header now matches this render: the body is W * nrows * 3)
  if (int rc = rt_nw_accum_reset(ctx, W, nrows)) return rc;
  if (int rc = rt_nw_accum_import(ctx, raw.data(), raw.size(), h.spp_done)) return rc;
  *spp_done = h.spp_done;
  return RT_OK;
}

// ---------------------------------------------------------------------------
// adaptive sampling (DESIGN.md §9 "Adaptive sampling")
// ---------------------------------------------------------------------------
// The adaptive accumulator holds, per pixel, the fixed-point colour sums, the sum of l^2 and the number n of samples
// behind them.  A pass gives every active pixel p the samples [n[p], n[p] + s_count): a sample's contribution
// depends on (seed, pixel, sample index) alone, so p's sums are those of a plain render of n[p] samples at p,
// whatever its neighbours received.
namespace {
constexpr int32_t kAdaptMaxSpp = 1 << 20;  // RT_NW_ADAPT_MAX_SPP: 192^2 * 2^28 * 2^20 < 2^64 keeps m2 from overflowing

size_t adapt_pixels(const rt_nw_ctx *c) { return size_t(c->adapt_W) * size_t(c->adapt_rows); }

int adapt_wait(rt_nw_ctx *ctx) {  // nothing of the context still running
  if (ctx->last_stream) HIP_TRY(hipStreamSynchronize(ctx->last_stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return RT_OK;
}
}  // namespace

RTMI_EXPORT int rt_nw_adapt_reset(rt_nw_ctx *ctx, int32_t W, int32_t nrows) {
  if (!ctx) return set_error(RT_EINVAL, "null ctx");
  if (W < 1 || nrows < 1 || int64_t(W) * nrows >= (int64_t(1) << 40))
    return set_error(RT_EINVAL, "rt_nw_adapt_reset: bad size %dx%d", W, nrows);
  Guard g(ctx->device);
  const size_t n = size_t(W) * size_t(nrows);
  if (int rc = adapt_wait(ctx)) return rc;
  if (ctx->adapt_cap < n) {
    ctx->adapt_cap = 0;
    ctx->adapt_W = ctx->adapt_rows = 0;
    int rc;
    if ((rc = alloc_copy<unsigned long long>(&ctx->adapt_sum, nullptr, n * 3)) ||
        (rc = alloc_copy<unsigned long long>(&ctx->adapt_m2, nullptr, n)) || (rc = alloc_copy<int32_t>(&ctx->adapt_n, nullptr, n)))
      return rc;
    ctx->adapt_cap = n;
  }
  ctx->adapt_W = W;
  ctx->adapt_rows = nrows;
  ctx->adapt_n_host.assign(n, 0);
  HIP_TRY(hipMemsetAsync(ctx->adapt_sum, 0, n * 3 * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(hipMemsetAsync(ctx->adapt_m2, 0, n * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(hipMemsetAsync(ctx->adapt_n, 0, n * sizeof(int32_t), ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return RT_OK;
}

RTMI_EXPORT int rt_nw_adapt_pass(rt_nw_ctx *ctx, const rt_nw_camera *cam, int32_t W, int32_t H, int32_t s_count,
                                 int32_t max_depth, uint64_t seed, int32_t row0, int32_t row_step, int32_t nrows,
                                 const uint8_t *active, void *stream) {
  const char *who = "rt_nw_adapt_pass";
  if (!ctx || !cam) return set_error(RT_EINVAL, "%s: null argument", who);
  if (s_count < 0 || s_count > kAdaptMaxSpp)
    return set_error(RT_EINVAL, "%s: bad sample count %d (a pixel holds at most 2^20 samples)", who, s_count);
  if (!ctx->adapt_sum || !ctx->adapt_W || W != ctx->adapt_W || nrows != ctx->adapt_rows)
    return set_error(RT_EINVAL, "%s: accumulator is not %dx%d (call rt_nw_adapt_reset)", who, W, nrows);
  if (adapt_pixels(ctx) > ctx->adapt_cap || ctx->adapt_n_host.size() != adapt_pixels(ctx))
    return set_error(RT_EHIP, "internal: adaptive accumulator too small");
  if (int rc = check_rows_args(ctx, cam, W, H, std::max(s_count, 1), max_depth, row0, row_step, nrows, 0, true, who)) return rc;
  // the work list: per tile with an active pixel inside the image, the mask of those pixels (bit ly * 8 + lx)
  const int32_t valid = std::min<int64_t>(nrows, (int64_t(H) - 1 - row0) / row_step + 1);
  const int32_t tiles_x = (W + 7) / 8, tiles_y = (valid + 7) / 8;
  std::vector<int32_t> tiles;
  std::vector<unsigned long long> masks;
  if (s_count > 0) {
    for (int32_t ty = 0; ty < tiles_y; ++ty)
      for (int32_t tx = 0; tx < tiles_x; ++tx) {
        unsigned long long m = 0;
        const int32_t vh = std::min(8, valid - ty * 8), vw = std::min(8, W - tx * 8);
        for (int32_t ly = 0; ly < vh; ++ly)
          for (int32_t lx = 0; lx < vw; ++lx) {
            const size_t p = size_t(ty * 8 + ly) * size_t(W) + size_t(tx * 8 + lx);
            if (active && !active[p]) continue;
            if (ctx->adapt_n_host[p] > kAdaptMaxSpp - s_count)
              return set_error(RT_EINVAL, "%s: pixel (%d, row %d) holds %d samples: %d more would pass 2^20", who, tx * 8 + lx,
                               ty * 8 + ly, ctx->adapt_n_host[p], s_count);
            m |= 1ull << (ly * 8 + lx);
          }
        if (m) {
          tiles.push_back(ty * tiles_x + tx);
          masks.push_back(m);
        }
      }
  }
  Guard g(ctx->device);
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  if (tiles.empty()) {  // nothing to sample: no launch, a count of zero segments
    if (int rc = take_turn(ctx, st)) return rc;
    MarkDone mark_done{ctx, st};
    HIP_TRY(hipMemsetAsync(ctx->segments, 0, sizeof(unsigned long long), st));
    return RT_OK;
  }
  // the list goes into the slot the pass before the last one used (that pass has to have ended: the host waits for
  // it alone), uploaded in stream order from the slot's host copy; the pass is asynchronous on `stream`
  rt_nw_ctx::AdaptList &L = ctx->adapt_list[ctx->adapt_slot];
  ctx->adapt_slot ^= 1;
  if (!L.done) HIP_TRY(hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
  if (L.used) HIP_TRY(hipEventSynchronize(L.done));
  L.used = false;
  const size_t nt = tiles.size();
  if (nt > L.cap) {
    L.cap = 0;
    int rc;
    if ((rc = alloc_copy<int32_t>(&L.tiles, nullptr, nt)) || (rc = alloc_copy<unsigned long long>(&L.masks, nullptr, nt))) return rc;
    L.cap = nt;
  }
  L.host_tiles.swap(tiles);
  L.host_masks.swap(masks);
  const std::vector<int32_t> &tiles_h = L.host_tiles;
  const std::vector<unsigned long long> &masks_h = L.host_masks;
  // (recorded whatever follows, so that the slot is not handed out again while a copy or the pass may still run)
  struct MarkSlot {
    rt_nw_ctx::AdaptList &l;
    hipStream_t s;
    ~MarkSlot() { l.used = hipEventRecord(l.done, s) == hipSuccess; }
  } mark_slot{L, st};
  HIP_TRY(hipMemcpyAsync(L.tiles, tiles_h.data(), nt * sizeof(int32_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(L.masks, masks_h.data(), nt * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
  AdaptLaunch al;
  al.dev.tiles = L.tiles;
  al.dev.masks = L.masks;
  al.dev.n = ctx->adapt_n;
  al.dev.m2 = ctx->adapt_m2;
  al.n_tiles = int32_t(nt);
  if (int rc = render_rows_impl(ctx, cam, W, H, s_count, max_depth, seed, row0, row_step, nrows, nullptr, stream, 0,
                                ctx->adapt_sum, who, &al))
    return rc;
  hipLaunchKernelGGL(adapt_advance_kernel, dim3(unsigned(nt)), dim3(64), 0, st, L.tiles, L.masks, ctx->adapt_n, W, tiles_x,
                     s_count);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ctx->last_done, st));  // (the pass ends with the counts)
  for (size_t k = 0; k < nt; ++k) {
    const int32_t ty = tiles_h[k] / tiles_x, tx = tiles_h[k] - ty * tiles_x;
    for (int b = 0; b < 64; ++b)
      if ((masks_h[k] >> b) & 1ull) ctx->adapt_n_host[size_t(ty * 8 + (b >> 3)) * size_t(W) + size_t(tx * 8 + (b & 7))] += s_count;
  }
  return RT_OK;
}

RTMI_EXPORT int rt_nw_adapt_export(rt_nw_ctx *ctx, int64_t *sum, uint64_t *m2, int32_t *n, size_t npix) {
  if (!ctx || !sum || !m2 || !n) return set_error(RT_EINVAL, "rt_nw_adapt_export: null argument");
  const size_t want = adapt_pixels(ctx);
  if (!ctx->adapt_sum || !want || npix != want)
    return set_error(RT_EINVAL, "rt_nw_adapt_export: %zu pixels, accumulator %zu (rt_nw_adapt_reset)", npix, want);
  Guard g(ctx->device);
  HIP_TRY(hipStreamSynchronize(ctx->last_stream ? ctx->last_stream : ctx->stream));
  HIP_TRY(hipMemcpy(sum, ctx->adapt_sum, npix * 3 * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(m2, ctx->adapt_m2, npix * sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(n, ctx->adapt_n, npix * sizeof(int32_t), hipMemcpyDeviceToHost));
  return RT_OK;
}

RTMI_EXPORT int rt_nw_adapt_import(rt_nw_ctx *ctx, const int64_t *sum, const uint64_t *m2, const int32_t *n, size_t npix) {
  if (!ctx || !sum || !m2 || !n) return set_error(RT_EINVAL, "rt_nw_adapt_import: null argument");
  const size_t want = adapt_pixels(ctx);
  if (!ctx->adapt_sum || !want || npix != want)
    return set_error(RT_EINVAL, "rt_nw_adapt_import: %zu pixels, accumulator %zu (call rt_nw_adapt_reset)", npix, want);
  for (size_t p = 0; p < npix; ++p)
    if (n[p] < 0 || n[p] > kAdaptMaxSpp) return set_error(RT_EINVAL, "rt_nw_adapt_import: sample count outside [0, 2^20]");
  Guard g(ctx->device);
  if (int rc = adapt_wait(ctx)) return rc;
  HIP_TRY(hipMemcpy(ctx->adapt_sum, sum, npix * 3 * sizeof(int64_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(ctx->adapt_m2, m2, npix * sizeof(uint64_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(ctx->adapt_n, n, npix * sizeof(int32_t), hipMemcpyHostToDevice));
  ctx->adapt_n_host.assign(n, n + npix);
  return RT_OK;
}

RTMI_EXPORT int rt_nw_adapt_resolve(rt_nw_ctx *ctx, float *dev_mean, float *host_mean, void *stream) {
  if (!ctx) return set_error(RT_EINVAL, "null ctx");
  if (!ctx->adapt_sum || !ctx->adapt_W) return set_error(RT_EINVAL, "rt_nw_adapt_resolve: no accumulator (rt_nw_adapt_reset)");
  if (!dev_mean && !host_mean) return set_error(RT_EINVAL, "rt_nw_adapt_resolve: no output");
  Guard g(ctx->device);
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  const size_t npix = adapt_pixels(ctx), n = npix * 3;
  float *out = dev_mean;
  if (!out) {  // through the context's float scratch, which renders share
    if (n > ctx->scratch_cap) {
      if (int rc = adapt_wait(ctx)) return rc;
      ctx->scratch_cap = 0;
      if (int rc = alloc_copy<float>(&ctx->scratch, nullptr, n)) return rc;
      ctx->scratch_cap = n;
    }
    out = ctx->scratch;
  }
  if (int rc = take_turn(ctx, st)) return rc;
  hipLaunchKernelGGL(adapt_resolve_kernel, dim3(unsigned((npix + 255) / 256)), dim3(256), 0, st, ctx->adapt_sum, ctx->adapt_n, out,
                     npix);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && host_mean) e = hipMemcpyAsync(host_mean, out, n * sizeof(float), hipMemcpyDeviceToHost, st);
  (void)hipEventRecord(ctx->last_done, st);
  if (e == hipSuccess && host_mean) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error(RT_EHIP, "rt_nw_adapt_resolve: %s", hipGetErrorString(e));
  return RT_OK;
}

namespace {
int adapt_header(rt_nw_scene *scene, const rt_nw_camera *cam, int32_t W, int32_t H, int32_t row0, int32_t row_step, int32_t nrows,
                 int32_t max_depth, uint64_t seed, CkptHeader &h) {
  h = CkptHeader{};
  if (int rc = rt_nw_scene_hash(scene, &h.scene_hash)) return rc;
  h.W = W;
  h.H = H;
  h.row0 = row0;
  h.row_step = row_step;
  h.nrows = nrows;
  h.max_depth = max_depth;
  h.seed = seed;
  h.camera_hash = camera_hash(cam);
  return RT_OK;
}
}  // namespace

RTMI_EXPORT int rt_nw_adapt_save(rt_nw_ctx *ctx, const char *path, rt_nw_scene *scene, const rt_nw_camera *cam, int32_t H,
                                 int32_t row0, int32_t row_step, int32_t max_depth, uint64_t seed) {
  if (!ctx || !path || !scene || !cam) return set_error(RT_EINVAL, "rt_nw_adapt_save: null argument");
  if (!ctx->adapt_sum || !ctx->adapt_W) return set_error(RT_EINVAL, "rt_nw_adapt_save: no accumulator (rt_nw_adapt_reset)");
  CkptHeader h;
  if (int rc = adapt_header(scene, cam, ctx->adapt_W, H, row0, row_step, ctx->adapt_rows, max_depth, seed, h)) return rc;
  const size_t npix = adapt_pixels(ctx);
  std::vector<int64_t> sum(npix * 3);
  std::vector<uint64_t> m2(npix);
  std::vector<int32_t> n(npix);
  if (int rc = rt_nw_adapt_export(ctx, sum.data(), m2.data(), n.data(), npix)) return rc;
  h.spp_done = *std::max_element(n.begin(), n.end());  // the largest count a pixel holds
  return adapt_ckpt_write(path, h, sum.data(), m2.data(), n.data());
}

RTMI_EXPORT int rt_nw_adapt_load(rt_nw_ctx *ctx, const char *path, rt_nw_scene *scene, const rt_nw_camera *cam, int32_t W,
                                 int32_t H, int32_t row0, int32_t row_step, int32_t nrows, int32_t max_depth, uint64_t seed) {
  if (!ctx || !path || !scene || !cam) return set_error(RT_EINVAL, "rt_nw_adapt_load: null argument");
  if (W < 1 || nrows < 1) return set_error(RT_EINVAL, "rt_nw_adapt_load: bad size %dx%d", W, nrows);
  CkptHeader want, h{};
  if (int rc = adapt_header(scene, cam, W, H, row0, row_step, nrows, max_depth, seed, want)) return rc;
  if (int rc = adapt_ckpt_read(path, h, nullptr, nullptr, nullptr)) return rc;
  if (h.W != W || h.H != H || h.row0 != row0 || h.row_step != row_step || h.nrows != nrows || h.max_depth != max_depth ||
      h.seed != seed || h.scene_hash != want.scene_hash || h.camera_hash != want.camera_hash)
    return set_error(RT_EINVAL, "rt_nw_adapt_load: %s was made for another render (size, rows, depth, seed, scene or camera)",
                     path);
  std::vector<int64_t> sum;
  std::vector<uint64_t> m2;
  std::vector<int32_t> n;
  if (int rc = adapt_ckpt_read(path, h, &sum, &m2, &n)) return rc;  // (the header matches this render: W * nrows pixels)
  for (int32_t v : n)
    if (v < 0 || v > kAdaptMaxSpp) return set_error(RT_EIO, "rt_nw_adapt_load: %s holds a bad sample count", path);
  if (int rc = rt_nw_adapt_reset(ctx, W, nrows)) return rc;
  return rt_nw_adapt_import(ctx, sum.data(), m2.data(), n.data(), n.size());
}

// The driver: pass, export, criterion, next mask, until nothing is active or the time limit passes.  The criterion
// runs on the host (rt_nw_adapt_criterion): the export of a W x nrows strip is small beside a pass.
RTMI_EXPORT int rt_nw_render_adaptive(rt_nw_ctx *ctx, rt_nw_scene *scene, const rt_nw_camera *cam, int32_t W, int32_t H,
                                      int32_t min_spp, int32_t max_spp, int32_t pass_spp, double threshold, double floor,
                                      int32_t dilate, int32_t max_depth, uint64_t seed, const char *checkpoint, double time_limit,
                                      float *mean_out, int32_t *n_out, double *err_out, rt_nw_adapt_stats *stats,
                                      rt_nw_adapt_on_pass on_pass, void *user) {
  const char *who = "rt_nw_render_adaptive";
  if (!ctx || !cam) return set_error(RT_EINVAL, "%s: null argument", who);
  if (checkpoint && !scene) return set_error(RT_EINVAL, "%s: a checkpoint needs the scene (its hash)", who);
  if (pass_spp < 1) return set_error(RT_EINVAL, "%s: pass_spp must be at least 1", who);
  if (W < 1 || H < 1 || int64_t(W) * H >= (int64_t(1) << 40)) return set_error(RT_EINVAL, "%s: bad size", who);
  const size_t npix = size_t(W) * size_t(H);
  std::vector<int64_t> sum(npix * 3);
  std::vector<uint64_t> m2(npix);
  std::vector<int32_t> n(npix);
  std::vector<uint8_t> active(npix);
  std::vector<double> err(npix);
  int64_t n_active = 0;
  // (the criterion's own checks of min_spp, max_spp, threshold, floor and dilate come first)
  if (int rc = rt_nw_adapt_criterion(sum.data(), m2.data(), n.data(), W, H, min_spp, max_spp, threshold, floor, dilate,
                                     active.data(), err.data(), &n_active))
    return rc;
  bool resumed = false;
  if (checkpoint) {
    if (FILE *probe = std::fopen(checkpoint, "rb")) {
      std::fclose(probe);
      if (int rc = rt_nw_adapt_load(ctx, checkpoint, scene, cam, W, H, 0, 1, H, max_depth, seed)) return rc;
      resumed = true;
    }
  }
  if (!resumed)
    if (int rc = rt_nw_adapt_reset(ctx, W, H)) return rc;
  if (stats) {
    stats->passes = 0;
    stats->stopped = 0;
    stats->total_samples = stats->pixels_at_max = stats->samples = stats->segments = 0;
  }
  const auto t0 = std::chrono::steady_clock::now();
  for (int32_t pass = 0;; ++pass) {
    if (int rc = rt_nw_adapt_export(ctx, sum.data(), m2.data(), n.data(), npix)) return rc;
    if (int rc = rt_nw_adapt_criterion(sum.data(), m2.data(), n.data(), W, H, min_spp, max_spp, threshold, floor, dilate,
                                       active.data(), err.data(), &n_active))
      return rc;
    if (n_active == 0) break;
    if (pass > 0 && time_limit >= 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() >= time_limit) {
      if (stats) stats->stopped = 1;  // (at least one pass always runs)
      break;
    }
    int32_t top = 0;  // no active pixel passes max_spp
    for (size_t p = 0; p < npix; ++p)
      if (active[p]) top = std::max(top, n[p]);
    const int32_t k = std::min(pass_spp, max_spp - top);
    if (int rc = rt_nw_adapt_pass(ctx, cam, W, H, k, max_depth, seed, 0, 1, H, active.data(), nullptr)) return rc;
    if (stats) {
      if (stats->active && pass < stats->cap) stats->active[pass] = n_active;
      stats->passes = pass + 1;
      uint64_t segs = 0;  // (waits for the pass, as the next export would)
      if (int rc = rt_nw_ctx_last_segments(ctx, &segs)) return rc;
      stats->segments += int64_t(segs);
      for (size_t p = 0; p < npix; ++p) stats->samples += active[p] ? k : 0;
    }
    if (checkpoint)  // (waits for the pass)
      if (int rc = rt_nw_adapt_save(ctx, checkpoint, scene, cam, H, 0, 1, max_depth, seed)) return rc;
    if (on_pass && on_pass(user, pass + 1, n_active)) {  // the caller ends the run: the state so far is returned
      if (stats) stats->stopped = 2;
      if (int rc = rt_nw_adapt_export(ctx, sum.data(), m2.data(), n.data(), npix)) return rc;
      if (int rc = rt_nw_adapt_criterion(sum.data(), m2.data(), n.data(), W, H, min_spp, max_spp, threshold, floor, dilate,
                                         active.data(), err.data(), &n_active))
        return rc;
      break;
    }
  }
  if (stats)
    for (size_t p = 0; p < npix; ++p) {
      stats->total_samples += n[p];
      stats->pixels_at_max += n[p] >= max_spp ? 1 : 0;
    }
  if (n_out) std::memcpy(n_out, n.data(), npix * sizeof(int32_t));
  if (err_out) std::memcpy(err_out, err.data(), npix * sizeof(double));
  if (mean_out)
    if (int rc = rt_nw_adapt_resolve(ctx, nullptr, mean_out, nullptr)) return rc;
  return RT_OK;
}

namespace {
// The validation kernels by walk (enum Walk), and the walk of the context's scene: its family's two-level walk,
// else the grid where the renders use it (grid), else the BVH.  A trace always walks the BVH.
const void *const kTraceKernels[kWalks] = {(const void *)trace_kernel<kWalkBvh>, nullptr, (const void *)trace_kernel<kWalkInst>,
                                           (const void *)trace_kernel<kWalkMove>, (const void *)trace_kernel<kWalkAffine>};
const void *const kHitsKernels[kWalks] = {(const void *)debug_hits_kernel<kWalkBvh>, (const void *)debug_hits_kernel<kWalkGrid>,
                                          (const void *)debug_hits_kernel<kWalkInst>, (const void *)debug_hits_kernel<kWalkMove>,
                                          (const void *)debug_hits_kernel<kWalkAffine>};
const void *const kRecordsKernels[kWalks] = {(const void *)debug_records_kernel<kWalkBvh>, (const void *)debug_records_kernel<kWalkGrid>,
                                             (const void *)debug_records_kernel<kWalkInst>, (const void *)debug_records_kernel<kWalkMove>,
                                             (const void *)debug_records_kernel<kWalkAffine>};
int walk_of(const rt_nw_ctx *ctx, bool grid) { return ctx->has_tri >= 3 ? kWalkInst + (ctx->has_tri - 3) : grid ? kWalkGrid : kWalkBvh; }

// rt_nw_debug_hits and rt_nw_debug_records (records): the rays up, one launch through the scene's walk, the results
// down.  out_aux: the box faces or the materials; out_pnuv: records only.
int debug_rays(rt_nw_ctx *ctx, const char *who, bool records, const float *rays, const uint64_t *keys, int32_t n, int32_t *out_id,
               float *out_t, int32_t *out_aux, float *out_pnuv) {
  if (!ctx || (n > 0 && (!rays || !out_id || !out_t || !out_aux || (records && !out_pnuv))) || n < 0)
    return set_error(RT_EINVAL, "%s: bad argument", who);
  if (ctx->nobj + ctx->nmed <= 0) return set_error(RT_EINVAL, "no scene uploaded (rt_nw_ctx_set_scene)");
  if (n == 0) return RT_OK;
  Guard g(ctx->device);
  const bool grid = accel_used(ctx) == RT_NW_ACCEL_GRID;
  const size_t lds = grid ? grid_bytes(ctx) : 0, count = size_t(n);
  if (lds > kCuLds) return set_error(RT_EUNSUPPORTED, "%s: grid of %zu B exceeds a CU's LDS", who, lds);
  DevBuf<float> d_rays, d_t, d_pnuv;
  DevBuf<unsigned long long> d_keys;
  DevBuf<int32_t> d_id, d_aux;
  hipError_t e = d_rays.upload(rays, count * 8);
  if (e == hipSuccess && keys) e = d_keys.upload(reinterpret_cast<const unsigned long long *>(keys), count);
  if (e == hipSuccess) e = d_t.alloc(count);
  if (e == hipSuccess) e = d_id.alloc(count);
  if (e == hipSuccess) e = d_aux.alloc(count);
  if (e == hipSuccess && records) e = d_pnuv.alloc(count * 8);
  if (e == hipSuccess) {
    View v = view_of(ctx);
    DebugRays q{d_rays.p, d_keys.p, n, ctx->nattr > 0 ? 1 : 0, d_id.p, d_t.p, d_aux.p, d_pnuv.p};
    void *args[] = {&v, &q};
    e = hipLaunchKernel((records ? kRecordsKernels : kHitsKernels)[walk_of(ctx, grid)], dim3(unsigned((n + 255) / 256)), dim3(256),
                        args, lds, ctx->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = d_id.download(out_id, count);
  if (e == hipSuccess) e = d_t.download(out_t, count);
  if (e == hipSuccess) e = d_aux.download(out_aux, count);
  if (e == hipSuccess && records) e = d_pnuv.download(out_pnuv, count * 8);
  if (e != hipSuccess) return set_error(RT_EHIP, "%s: %s", who, hipGetErrorString(e));
  return RT_OK;
}
}  // namespace

RTMI_EXPORT int rt_nw_debug_trace(rt_nw_ctx *ctx, const rt_nw_camera *cam, int32_t W, int32_t H, int32_t max_depth,
                                  uint64_t seed, int32_t i, int32_t j, int32_t s, float *rec, int32_t cap, int32_t *n) {
  if (!ctx || !cam || !rec || !n || cap < 1 || max_depth < 1 || i < 0 || i >= W || j < 0 || j >= H)
    return set_error(RT_EINVAL, "rt_nw_debug_trace: bad argument");
  Guard g(ctx->device);
  View v = view_of(ctx);
  Args a = camera_args(cam, W, H, max_depth, seed);
  int has_attr = ctx->nattr > 0 ? 1 : 0;
  DevBuf<float> d_rec;
  DevBuf<int32_t> d_n;
  HIP_TRY(d_rec.alloc(size_t(cap) * 12));
  HIP_TRY(d_n.alloc(1));
  void *args[] = {&v, &a, &i, &j, &s, &d_rec.p, &cap, &d_n.p, &has_attr};
  hipError_t e = hipLaunchKernel(kTraceKernels[walk_of(ctx, false)], dim3(1), dim3(64), args, 0, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = d_n.download(n, 1);
  if (e == hipSuccess) e = d_rec.download(rec, size_t(*n) * 12);
  if (e != hipSuccess) return set_error(RT_EHIP, "rt_nw_debug_trace: %s", hipGetErrorString(e));
  return RT_OK;
}

RTMI_EXPORT int rt_nw_debug_trace_t(rt_nw_ctx *ctx, const rt_nw_camera *cam, int32_t W, int32_t H, int32_t max_depth,
                                    uint64_t seed, int32_t i, int32_t j, int32_t s, float *rec, int32_t cap, int32_t *n,
                                    float *time) {
  if (!time) return set_error(RT_EINVAL, "rt_nw_debug_trace_t: null time");
  if (int rc = rt_nw_debug_trace(ctx, cam, W, H, max_depth, seed, i, j, s, rec, cap, n)) return rc;
  Guard g(ctx->device);
  DevBuf<float> d_time;
  HIP_TRY(d_time.alloc(1));
  hipLaunchKernelGGL(trace_time_kernel, dim3(1), dim3(64), 0, ctx->stream, camera_args(cam, W, H, max_depth, seed), i, j, s, d_time.p);
  hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = d_time.download(time, 1);
  if (e != hipSuccess) return set_error(RT_EHIP, "rt_nw_debug_trace_t: %s", hipGetErrorString(e));
  return RT_OK;
}

RTMI_EXPORT int rt_nw_ctx_scene_tri(rt_nw_ctx *ctx, int32_t *tri) {
  if (!ctx || !tri) return set_error(RT_EINVAL, "null");
  *tri = ctx->has_tri;
  return RT_OK;
}

RTMI_EXPORT int rt_nw_debug_hits(rt_nw_ctx *ctx, const float *rays, const uint64_t *keys, int32_t n, int32_t *out_id,
                                 float *out_t, int32_t *out_face) {
  return debug_rays(ctx, "rt_nw_debug_hits", false, rays, keys, n, out_id, out_t, out_face, nullptr);
}

RTMI_EXPORT int rt_nw_debug_records(rt_nw_ctx *ctx, const float *rays, const uint64_t *keys, int32_t n, int32_t *out_id,
                                    float *out_t, float *out_pnuv, int32_t *out_mat) {
  return debug_rays(ctx, "rt_nw_debug_records", true, rays, keys, n, out_id, out_t, out_mat, out_pnuv);
}

// ---------------------------------------------------------------------------
// denoising (DESIGN.md §9 "Denoising"): the feature buffers and the driver; the filter is rtmi_nw_denoise.hip
// ---------------------------------------------------------------------------
namespace {
const void *const kFeaturesKernels[kWalks] = {(const void *)features_kernel<kWalkBvh>, (const void *)features_kernel<kWalkGrid>,
                                              (const void *)features_kernel<kWalkInst>, (const void *)features_kernel<kWalkMove>,
                                              (const void *)features_kernel<kWalkAffine>};
}  // namespace

RTMI_EXPORT int rt_nw_render_features(rt_nw_ctx *ctx, const rt_nw_camera *cam, int32_t W, int32_t H, int32_t fspp, uint64_t seed,
                                      float *dev_feat, float *host_feat, void *stream) {
  const char *who = "rt_nw_render_features";
  if (int rc = check_rows_args(ctx, cam, W, H, 1, 1, 0, 1, std::max(H, 1), 0, false, who)) return rc;
  if (!dev_feat && !host_feat) return set_error(RT_EINVAL, "%s: no output", who);
  if (fspp < 1 || fspp > 1024) return set_error(RT_EINVAL, "%s: fspp %d outside 1..1024", who, fspp);
  if (int64_t(W) * H >= (int64_t(1) << 31)) return set_error(RT_EINVAL, "%s: more than 2^31 pixels", who);
  Guard g(ctx->device);
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  const bool grid = accel_used(ctx) == RT_NW_ACCEL_GRID;
  const size_t lds = grid ? grid_bytes(ctx) : 0, npix = size_t(W) * size_t(H), n = npix * 8;
  if (lds > kCuLds) return set_error(RT_EUNSUPPORTED, "%s: grid of %zu B exceeds a CU's LDS", who, lds);
  float *out = dev_feat;
  if (!out) {  // through the context's float scratch, which renders share
    if (n > ctx->scratch_cap) {
      if (int rc = adapt_wait(ctx)) return rc;
      ctx->scratch_cap = 0;
      if (int rc = alloc_copy<float>(&ctx->scratch, nullptr, n)) return rc;
      ctx->scratch_cap = n;
    }
    out = ctx->scratch;
  }
  if (int rc = take_turn(ctx, st)) return rc;
  View v = view_of(ctx);
  Args a = camera_args(cam, W, H, 1, seed);
  FeatArgs f{fspp, ctx->nattr > 0 ? 1 : 0, out};
  void *args[] = {&v, &a, &f};
  hipError_t e = hipLaunchKernel(kFeaturesKernels[walk_of(ctx, grid)], dim3(unsigned((npix + 255) / 256)), dim3(256), args, lds, st);
  if (e == hipSuccess && host_feat) e = hipMemcpyAsync(host_feat, out, n * sizeof(float), hipMemcpyDeviceToHost, st);
  (void)hipEventRecord(ctx->last_done, st);
  if (e == hipSuccess && host_feat) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error(RT_EHIP, "%s: %s", who, hipGetErrorString(e));
  return RT_OK;
}

// the denoiser's side of the context (rtmi_nw_internal.h)
namespace rtmi {
namespace nw {
int ctx_link(rt_nw_ctx *ctx, CtxLink &out) {
  if (!ctx) return set_error(RT_EINVAL, "null ctx");
  out.device = ctx->device;
  out.stream = ctx->stream;
  out.scratch = &ctx->denoise;
  return RT_OK;
}
int ctx_begin(rt_nw_ctx *ctx, void *stream) { return take_turn(ctx, static_cast<hipStream_t>(stream)); }
void ctx_end(rt_nw_ctx *ctx, void *stream) { (void)hipEventRecord(ctx->last_done, static_cast<hipStream_t>(stream)); }
int ctx_idle(rt_nw_ctx *ctx) { return adapt_wait(ctx); }
}  // namespace nw
}  // namespace rtmi

RTMI_EXPORT int rt_nw_render_denoised(rt_nw_ctx *ctx, rt_nw_scene *scene, const rt_nw_camera *cam, int32_t W, int32_t H,
                                      int32_t min_spp, int32_t max_spp, int32_t pass_spp, double threshold, double floor,
                                      int32_t dilate, int32_t max_depth, uint64_t seed, const char *checkpoint, double time_limit,
                                      float *mean_out, int32_t *n_out, double *err_out, rt_nw_adapt_stats *stats,
                                      rt_nw_adapt_on_pass on_pass, void *user, int32_t fspp, const rt_nw_denoise_params *p,
                                      float *denoised_out) {
  const char *who = "rt_nw_render_denoised";
  if (!denoised_out) return set_error(RT_EINVAL, "%s: null denoised_out", who);
  if (fspp < 1 || fspp > 1024) return set_error(RT_EINVAL, "%s: fspp %d outside 1..1024", who, fspp);
  if (p)
    if (int rc = rt_nw_denoise_params_check(p)) return rc;
  if (int rc = rt_nw_render_adaptive(ctx, scene, cam, W, H, min_spp, max_spp, pass_spp, threshold, floor, dilate, max_depth, seed,
                                     checkpoint, time_limit, mean_out, n_out, err_out, stats, on_pass, user))
    return rc;
  if (int64_t(W) * H >= (int64_t(1) << 31)) return set_error(RT_EINVAL, "%s: more than 2^31 pixels", who);
  Guard g(ctx->device);
  const size_t npix = size_t(W) * size_t(H);
  std::vector<int64_t> sum(npix * 3);
  std::vector<uint64_t> m2(npix);
  std::vector<int32_t> n(npix);
  std::vector<float> var(npix);
  if (int rc = rt_nw_adapt_export(ctx, sum.data(), m2.data(), n.data(), npix)) return rc;
  if (int rc = rt_nw_adapt_variance(sum.data(), m2.data(), n.data(), W, H, var.data())) return rc;
  // one device allocation: mean (in place the filtered image) | var | feat
  DevBuf<float> d;
  HIP_TRY(d.alloc(npix * 12));
  float *d_mean = d.p, *d_var = d.p + 3 * npix, *d_feat = d.p + 4 * npix;
  HIP_TRY(hipMemcpyAsync(d_var, var.data(), npix * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  int rc = rt_nw_adapt_resolve(ctx, d_mean, nullptr, nullptr);
  if (rc == RT_OK) rc = rt_nw_render_features(ctx, cam, W, H, fspp, seed, d_feat, nullptr, nullptr);
  if (rc == RT_OK) rc = rt_nw_denoise(ctx, W, H, d_mean, d_var, d_feat, p, d_mean, nullptr, nullptr);
  hipError_t e = hipSuccess;
  if (rc == RT_OK) e = hipMemcpyAsync(denoised_out, d_mean, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);  // (before the allocation and var go)
  if (rc != RT_OK) return rc;
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return set_error(RT_EHIP, "%s: %s", who, hipGetErrorString(e));
  return RT_OK;
}

// Analysis builds only (RTMI_NW_PHASES): the phase cycle sums since the last
// call (see g_nw_phase), zeroed after reading; RT_EUNSUPPORTED otherwise.
// RTMI_STATS build (librtmi_stats.so): the executed-work counters of the
// launches since the last call (see g_nw_stats), zeroed after reading;
// RT_EUNSUPPORTED in the product build.
RTMI_EXPORT int rt_nw_debug_counters(uint64_t *out4) {
#if RTMI_STATS
  if (!out4) return set_error(RT_EINVAL, "null");
  HIP_TRY(hipDeviceSynchronize());
  unsigned long long v[4] = {0, 0, 0, 0}, z[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyFromSymbol(v, HIP_SYMBOL(g_nw_stats), sizeof v));
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_nw_stats), z, sizeof z));
  for (int q = 0; q < 4; ++q) out4[q] = v[q];
  return RT_OK;
#else
  (void)out4;
  return set_error(RT_EUNSUPPORTED, "rt_nw_debug_counters: not an RTMI_STATS build");
#endif
}

RTMI_EXPORT int rt_nw_debug_phases(uint64_t *out4) {
#if RTMI_NW_PHASES
  if (!out4) return set_error(RT_EINVAL, "null");
  HIP_TRY(hipDeviceSynchronize());
  unsigned long long v[4];
  HIP_TRY(hipMemcpyFromSymbol(v, HIP_SYMBOL(g_nw_phase), sizeof v));
  for (int q = 0; q < 4; ++q) out4[q] = v[q];
  const unsigned long long z[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_nw_phase), z, sizeof z));
  return RT_OK;
#else
  (void)out4;
  return set_error(RT_EUNSUPPORTED, "rt_nw_debug_phases: not an RTMI_NW_PHASES build");
#endif
}

RTMI_EXPORT int rt_nw_ctx_last_kernel(rt_nw_ctx *ctx, int32_t *out4) {
  if (!ctx || !out4) return set_error(RT_EINVAL, "null");
  for (int q = 0; q < 4; ++q) out4[q] = ctx->last_kernel[q];
  return RT_OK;
}

RTMI_EXPORT int rt_nw_ctx_last_staging(rt_nw_ctx *ctx, int32_t *out2) {
  if (!ctx || !out2) return set_error(RT_EINVAL, "null");
  out2[0] = ctx->last_staging[0];
  out2[1] = ctx->last_staging[1];
  return RT_OK;
}

RTMI_EXPORT int rt_nw_ctx_last_segments(rt_nw_ctx *ctx, uint64_t *segments) {
  if (!ctx || !segments) return set_error(RT_EINVAL, "null");
  Guard g(ctx->device);
  unsigned long long v = 0;
  HIP_TRY(hipDeviceSynchronize());  // the render may have run on a caller's stream
  HIP_TRY(hipMemcpy(&v, ctx->segments, sizeof v, hipMemcpyDeviceToHost));
  *segments = v;
  return RT_OK;
}
