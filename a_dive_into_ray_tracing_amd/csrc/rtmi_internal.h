// rtmi_internal.h — shared between the host (rtmi_host.cpp,
// rtmi_accel_build.cpp) and device (rtmi_device.hip) halves of librtmi.so:
// the error state, and what rtmi_accel_build.cpp builds on the CPU for
// rt_ctx_set_scene (rtmi_device.hip) to upload.  Not installed.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/rtmi.h"
#include "rtmi_accel.h"

#define RTMI_EXPORT extern "C" __attribute__((visibility("default")))

namespace rtmi {
int set_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void clear_error();

// FNV-1a-64 (the checkpoint header's scene and camera hashes, rt_debug_accel_digest)
constexpr uint64_t kFnvBasis = 14695981039346656037ull;
inline uint64_t fnv1a(uint64_t h, const void *p, size_t n) {
  const unsigned char *b = static_cast<const unsigned char *>(p);
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

inline Cam<float> cam_f(const rt_camera *c) {
  auto v = [](const double *p) { return mk(float(p[0]), float(p[1]), float(p[2])); };
  return Cam<float>{v(c->origin), v(c->lower_left_corner), v(c->horizontal), v(c->vertical), v(c->u), v(c->v),
                    float(c->lens_radius)};
}
inline Cam<double> cam_d(const rt_camera *c) {
  auto v = [](const double *p) { return mk(p[0], p[1], p[2]); };
  return Cam<double>{v(c->origin), v(c->lower_left_corner), v(c->horizontal), v(c->vertical), v(c->u), v(c->v),
                     c->lens_radius};
}

// a record of the double path (uploaded as double4)
struct Rec4d {
  double x, y, z, w;
};
static_assert(sizeof(Rec4d) == 32, "a double record is one double4");

// Everything rt_ctx_set_scene uploads for a scene, built on the CPU
// (rtmi_accel_build.cpp build_accel).  Sizes only: whether a structure is
// staged in LDS is the launch side's decision (it depends on the block shape).
struct AccelBuild {
  // geom[k]  = {cx, cy, cz, |c|^2 - r^2} (float path) / {cx, cy, cz, r*r} (double path)
  // shade0[k] = {1/r, albedo r, g, b}
  // shade1[k] = {kind, fuzz (clamped), ir, 1/ir}
  // (g: n + kGeomPad records, zeros behind the scene's)
  std::vector<Rec4> g, s0, s1;
  std::vector<Rec4d> g64, s064, s164;
  // the big spheres' slots: their scene indices in ascending order, padded
  // with -1 (never-hit dummies) to a multiple of 2 kBigGroup; empty: none
  std::vector<int32_t> big_slots;
  int32_t nbig = 0;
  // BVH over the small spheres: nodes in DFS order, the
  // spheres' records in leaf order and their scene indices
  std::vector<BvhNode> nodes;
  std::vector<Rec4> bvh_sph;
  std::vector<int32_t> bvh_idx;
  // uniform grid over the same spheres (its sphere array is g
  // by scene index).  has_grid false: the scene has none.  grid.cells and
  // grid.refs are left null (device pointers, set at the upload)
  bool has_grid = false;
  GridDesc grid{};
  std::vector<uint32_t> cells;  // ncells + 1: each cell's first reference
  std::vector<uint32_t> refs;   // 16 x scene index
  // tile lists, in the upload layout: {centre, grown radius}
  // per small sphere (ntile), then one uint32 per sphere, a record slot of it
  // (offset from the first slot / 16), padded to whole records, then {centre,
  // grown radius} per big sphere in slot order (ntile_big; 0 for more than
  // kTileBigMax).  Empty when a slot number passes 16 bits.
  std::vector<Rec4> tile_tab;
  int32_t ntile = 0, ntile_big = 0;
};
// RT_OK, or the error set (an unsupported material kind)
int build_accel(const rt_scene *scene, AccelBuild &out);
// The image stage_grid builds in LDS, offsets from 0 (grid_lds_bytes), for a
// grid walked in global memory
std::vector<char> grid_image(const AccelBuild &ab);
}  // namespace rtmi
