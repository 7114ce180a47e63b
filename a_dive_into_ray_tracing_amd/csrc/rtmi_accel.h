// rtmi_accel.h — what the host builders (rtmi_accel_build.cpp) and the kernels
// (rtmi_path.h, rtmi_device.hip) must agree on about the RTIOW acceleration
// structures: the record and node types, the grid descriptor, the LDS layouts'
// byte counts, the tile geometry and the tile lists' bundle test.  Plain C++ so
// that a host translation unit, and a sanitizer build of it, compiles the very
// code the kernels run; nothing of the HIP runtime is included.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTMI_HD __host__ __device__
#else
#define RTMI_HD
#endif

namespace rtmi {

constexpr int kGeomPad = 16;  // zero spheres after the scene's geom records (padding)

// One 16-byte record of a host-built array ({cx, cy, cz, S} of a sphere, a
// shading record, {centre, grown radius} of a tile table); the device side
// uploads the arrays as float4.
struct alignas(16) Rec4 {
  float x, y, z, w;
};
static_assert(sizeof(Rec4) == 16, "a record is one float4");

template <class R> struct V3 { R x, y, z; };
template <class R> RTMI_HD inline __attribute__((always_inline)) V3<R> mk(R x, R y, R z) { return V3<R>{x, y, z}; }

template <class R> struct Cam {
  V3<R> origin, llc, hor, ver, u, v;
  R lens;
};

// ---------------------------------------------------------------------------
// BVH over the small spheres
// ---------------------------------------------------------------------------
// One node = 16 bytes = one ds_read_b128: per axis the box's lo and hi as
// IEEE halves in one dword (lo in bits 0-15), rounded OUTWARD from the
// double bounds (a half box contains the float box it replaces, so culling
// stays conservative; the slab test converts them for free with
// v_fma_mix_f32), and a link: >= 0 for an inner node = the skip index (next
// node when the box is missed; the first child is index + 1), < 0 for a
// leaf = ~(first << 4 | count) (the next node is index + 1 either way).
struct BvhNode {
  uint32_t x, y, z;
  int32_t link;
};
static_assert(sizeof(BvhNode) == 16, "BVH node is one 16-byte LDS read");
#ifndef RTMI_BVH_LEAF
#define RTMI_BVH_LEAF 4
#endif
constexpr int kLeafMax = RTMI_BVH_LEAF;
#ifndef RTMI_BIG_FACTOR
#define RTMI_BIG_FACTOR 4
#endif
#ifndef RTMI_BIG_GROUP
#define RTMI_BIG_GROUP 2
#endif
constexpr int kBigGroup = RTMI_BIG_GROUP;  // sphere pairs per step of the big-sphere loop
static_assert(kLeafMax >= 1 && kLeafMax <= 15, "leaf size");

// The BVH lives in LDS during a launch (dynamic shared memory, staged by
// every block at its start): the traversal is a chain of dependent node
// loads, ~100 cycles from LDS against ~500+ from L2.  Layout: nnodes 16-byte
// nodes, then nsph sphere float4s, then nsph uint16 scene indices (the BVH is
// only offered for scenes of < 65536 spheres).
RTMI_HD constexpr size_t bvh_lds_bytes(int32_t nnodes, int32_t nsph) {
  return size_t(nnodes + nsph) * 16 + size_t(nsph) * 2;
}

// ---------------------------------------------------------------------------
// uniform grid over the small spheres (RT_ACCEL_GRID)
// ---------------------------------------------------------------------------
// Cells of size h over the box g0 + [0, n*h) of the spheres' margin-grown
// boxes.  Cell c lists refs[cells[c] .. cells[c+1]): every sphere whose grown
// box overlaps it, as 16 x its scene index.  In LDS (stage_grid) each reference
// becomes a copy of its sphere's record, so the walk reads a sphere with one
// ds_read_b128 at the reference itself (grid_lds_bytes).
struct GridDesc {
  float g0[3], h[3], inv_h[3], g1[3];  // origin, cell size, 1/h, far corner
  int32_t n[3];
  int32_t ncells, nrefs;
  const uint32_t *cells;  // ncells + 1 first-reference indices
  const uint32_t *refs;
  uint32_t cells_off, idx_off;  // in LDS: the cell starts and the slot indices, bytes past the slots
  // the cell-start table's strides in bytes, 4 n0 and 4 n0 n1 (grid_strides):
  // the walk forms a cell's address with 24-bit multiplies by these
  uint32_t row_bytes, layer_bytes;
  float nm1[3];  // n - 1 as floats: the entry cell's clamp
};

// The strides of the cell-start table.  The walk multiplies them by cell
// coordinates with v_mul_u32_u24, which reads 24 bits of each operand: the
// coordinates must stay below 2^16 and the strides below 2^24, or the grid is
// refused (false).
inline bool grid_strides(GridDesc &g) {
  for (int a = 0; a < 3; ++a)
    if (g.n[a] < 1 || g.n[a] >= (1 << 16)) return false;
  const uint64_t row = 4ull * uint64_t(g.n[0]), layer = row * uint64_t(g.n[1]);
  if (layer >= (1ull << 24)) return false;
  g.row_bytes = uint32_t(row);
  g.layer_bytes = uint32_t(layer);
  for (int a = 0; a < 3; ++a) g.nm1[a] = float(g.n[a] - 1);
  return true;
}

// Grid LDS layout ("record slots"): one 16-byte sphere record {c, S} per slot
// — first the big spheres' slots (2 x nbig_pairs, dummies included), then
// every cell's references in cell order, each a copy of the record of the
// sphere it lists — then ncells + 1 uint32 cell starts (the LDS addresses of
// their first slots), then one uint16 scene index per slot.  The walk reads a
// sphere with one ds_read_b128 at the slot (no reference indirection), and
// names a hit by its slot's LDS address (a "key"); the scene index is read
// from the index table only for an exact tie and once at the walk's end.
RTMI_HD constexpr size_t grid_lds_bytes(int32_t nbig_slots, int32_t ncells, int32_t nrefs) {
  return size_t(nbig_slots + nrefs) * 16 + (size_t(ncells) + 1) * 4 + (size_t(nbig_slots + nrefs) * 2 + 3) / 4 * 4;
}

// ---------------------------------------------------------------------------
// tiles, and the spheres a tile's camera rays can meet
// ---------------------------------------------------------------------------
// Automatic tile shape: 8x8 unless 16x4 leaves fewer idle lanes in partial
// tiles.  A 100-row strip (1/8 of config 2's rows) fills 25 rows of 16x4 tiles
// but 12.5 of 8x8: 7.04 vs 7.16 ms, while the whole frame runs 50.6 ms with 8x8
// and 50.9 with 16x4 (profiles/r01/session6/tile_ab.txt).
inline int auto_tile_w(int32_t W, int32_t rows) {
  auto idle = [&](int64_t tw) {
    const int64_t th = 64 / tw;
    return ((W + tw - 1) / tw) * tw * ((rows + th - 1) / th) * th - int64_t(W) * rows;
  };
  return idle(16) < idle(8) ? 16 : 8;
}

// The rows and columns of tile `tile` of a strip (render_kernel's item
// geometry): columns [x0, x0 + vw), image rows j_lo .. j_hi
inline void tile_extent(int32_t W, int32_t row0, int32_t row_step, int32_t nvalid, int32_t tw, int32_t tile,
                        int32_t &x0, int32_t &vw, int32_t &j_lo, int32_t &j_hi) {
  const int32_t th = 64 / tw, tiles_x = (W + tw - 1) / tw, ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int32_t y0 = ty * th, vh = std::min(th, nvalid - y0);
  x0 = tx * tw;
  vw = std::min(tw, W - x0);
  j_lo = row0 + y0 * row_step;
  j_hi = row0 + (y0 + vh - 1) * row_step;
}

// The camera rays of one tile — lens points o = origin + lens (px u + py v),
// (px, py) in the unit disk, through F(s, t) = llc + s hor + t ver with (s, t)
// in the tile's rectangle — as a cone of balls around one central ray: every
// point of every such ray lies within rho + tau k of the central point
// origin + tau e (tau >= 0 the distance along the unit axis e).  Host and
// kernel run this same code (rt_debug_tile_list, render_kernel).
struct TileBundle {
  float ox, oy, oz;  // the camera origin
  float ex, ey, ez;  // the axis: unit(Fc - origin), Fc the mean of F's four corners
  float rho;         // the lens disk's radius in space, with the margins below
  float k;           // (Rf + rho) / |Fc - origin|, Rf the largest corner distance from Fc, with the margins
  float q;           // max(0, 1 - k^2)
};
constexpr int kTileListCap = 32;      // entries of a wave's list (16 bits each)
constexpr int kTileListMinSpp = 4;    // items of fewer samples build no list (the 1-spp cost probe)
// Big spheres in the lists: a scene of at most kTileBigMax big spheres has
// them tested against the tile's bundle too (one more round of the build), and
// the ones that pass are appended to the tile's list as their record slots'
// keys (slot j's is j).  kTileBigFlag in the tile_list value says so: the list
// then names every sphere a camera ray of the tile can meet, and the batch
// runs no hit_big.  The value's bits: 0-5 the length, 6-21 the LDS address
// (below 2^16), 30 the flag.
constexpr int kTileBigMax = 8;
constexpr int32_t kTileBigFlag = 1 << 30;

// The tile of columns [x0, x0 + vw) and image rows j_lo .. j_hi (a strip's
// rows lie row_step apart: any rows between them are covered too).  The
// jitter is in [0, 1), so s spans [x0, x0 + vw] / (W - 1) and t
// [j_lo, j_hi + 1] / (H - 1).
RTMI_HD inline TileBundle tile_bundle(const Cam<float> &c, int32_t W, int32_t H, int32_t x0, int32_t vw,
                                      int32_t j_lo, int32_t j_hi) {
  const float s0 = float(x0) / float(W - 1), s1 = float(x0 + vw) / float(W - 1);
  const float t0 = float(j_lo) / float(H - 1), t1 = float(j_hi + 1) / float(H - 1);
  // F is affine in (s, t): Fc at the rectangle's centre, the corners at
  // +-a +-b from it (a, b half the rectangle's sides in space)
  const float sc = 0.5f * (s0 + s1), tc = 0.5f * (t0 + t1), sh = 0.5f * (s1 - s0), th = 0.5f * (t1 - t0);
  const float dx = c.llc.x + sc * c.hor.x + tc * c.ver.x - c.origin.x;
  const float dy = c.llc.y + sc * c.hor.y + tc * c.ver.y - c.origin.y;
  const float dz = c.llc.z + sc * c.hor.z + tc * c.ver.z - c.origin.z;
  const float ax = sh * c.hor.x, ay = sh * c.hor.y, az = sh * c.hor.z;
  const float bx = th * c.ver.x, by = th * c.ver.y, bz = th * c.ver.z;
  const float aa = ax * ax + ay * ay + az * az, bb = bx * bx + by * by + bz * bz, ab = ax * bx + ay * by + az * bz;
  const float rf = sqrtf(aa + bb + 2.0f * fabsf(ab));  // max |+-a +-b|
  // |px u + py v|^2 <= the larger eigenvalue of [[u.u, u.v], [u.v, v.v]] on the unit disk
  const float uu = c.u.x * c.u.x + c.u.y * c.u.y + c.u.z * c.u.z, vv = c.v.x * c.v.x + c.v.y * c.v.y + c.v.z * c.v.z;
  const float uv = c.u.x * c.v.x + c.u.y * c.v.y + c.u.z * c.v.z;
  const float hd = 0.5f * (uu - vv);
  const float rho = fabsf(c.lens) * sqrtf(0.5f * (uu + vv) + sqrtf(hd * hd + uv * uv));
  const float len = sqrtf(dx * dx + dy * dy + dz * dz), inv = 1.0f / len;
  TileBundle b;
  b.ox = c.origin.x; b.oy = c.origin.y; b.oz = c.origin.z;
  b.ex = dx * inv; b.ey = dy * inv; b.ez = dz * inv;
  // Margins that dwarf float error (the rays the kernel forms differ from the
  // ideal ones by ~1e-6 of the coordinates' scale): 1e-3 relative on the whole
  // bound, and 1e-5 of the origin's scale and of the distance along the axis
  const float on = fmaxf(fmaxf(fabsf(c.origin.x), fabsf(c.origin.y)), fabsf(c.origin.z));
  b.rho = 1.001f * rho + 1e-5f * (1.0f + on);
  b.k = 1.001f * ((rf + rho) * inv) + 1e-5f;
  b.q = fmaxf(0.0f, 1.0f - b.k * b.k);
  return b;
}

// Whether a ray of the bundle can meet the sphere (centre, radius rg: the
// grown radius, tile_sphere_radius).  With tau_c = max(0, (c - origin).e) and
// h the distance from c to the axis point at tau_c, every ball of the cone
// lies in h sqrt(1 - k^2) <= rg + rho + k tau_c; the test
// passes unless that fails, so a NaN (a degenerate camera) or k >= 1 (a huge
// aperture, a tiny image: q = 0) passes everything.  Conservative only: it
// adds spheres to a list, it never decides a hit.
RTMI_HD inline bool tile_may_hit(const TileBundle &b, float cx, float cy, float cz, float rg) {
  const float px = cx - b.ox, py = cy - b.oy, pz = cz - b.oz;
  const float al = px * b.ex + py * b.ey + pz * b.ez;
  const float tau = fmaxf(al, 0.0f);
  const float qx = px - tau * b.ex, qy = py - tau * b.ey, qz = pz - tau * b.ez;
  const float h2 = qx * qx + qy * qy + qz * qz;
  const float rhs = rg + b.rho + b.k * tau;
  return !(h2 * b.q > rhs * rhs);
}

}  // namespace rtmi
