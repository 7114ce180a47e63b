// rtmi_nw_internal.h — host-side interface between the Next-Week scene
// builder (rtmi_nw_scene.cpp) and the device half (rtmi_nw.hip).  Not installed.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/rtmi_nw.h"
#include "rtmi_nw_types.h"

namespace rtmi {
namespace nw {

// BVH node over objects: DFS order with skip links (the RTIOW BVH's format,
// rtmi_accel.h BvhNode): leaf = first << 4 | count, -1 for inner nodes.
struct Node {
  float bmin[3];
  int32_t skip;
  float bmax[3];
  int32_t leaf;
};

// What the device renders: flattened records in BVH leaf order, plus each
// object's world-insertion index (the tie-break key).
struct DeviceScene {
  std::vector<Obj> obj;          // non-media objects, BVH leaf order; aux = twin medium's index in med + 1
  std::vector<int32_t> obj_id;   // insertion index of obj[k]
  std::vector<TriAttr> attr;     // triangle attribute records (rt_nw_mesh_attr); empty when no object has one
  std::vector<int32_t> obj_attr; // record of obj[k] or -1; empty when no object has one
  std::vector<Obj> med;          // media, insertion order
  std::vector<int32_t> med_id;   // their insertion indices
  std::vector<Inst> inst;
  std::vector<Mat> mat;
  std::vector<Tex> tex;
  std::vector<float> perlin_vec;     // n_perlin * 256 * 4
  std::vector<int32_t> perlin_perm;  // n_perlin * 768
  std::vector<uint8_t> image_px;
  std::vector<Image> image;
  std::vector<Node> nodes;
  float background[3];
  bool has_media;
  // uniform grid over the same objects; grid_ok false when
  // the scene has none (no small objects, or it would not fit in LDS)
  bool grid_ok = false;
  float grid_g0[3], grid_h[3], grid_inv_h[3], grid_g1[3];
  int32_t grid_n[3];
  int32_t grid_max_cell = 0;               // largest cell's object count
  std::vector<uint16_t> grid_cell_start;   // ncells + 1
  std::vector<uint16_t> grid_refs;         // object indices (leaf order) per cell
  std::vector<int32_t> grid_big;           // objects tested brute force beside the grid (leaf order)
  // Shared meshes (rt_nw_shared, DESIGN.md §9 "Shared meshes"); all empty in a
  // scene without a placement.  Each placement is one kInstance record in obj
  // (alone in its top-level leaf; obj_id = first(p)); the triangles of every
  // placed mesh sit once in the pool, in the leaf order of that mesh's
  // bottom-level BVH.  bnodes' skip links and leaf ranges are absolute: indices
  // into bnodes and into pool, each inside its mesh's ranges.
  struct SharedMesh {
    int32_t node0, n_nodes;  // its bottom-level BVH in bnodes
    int32_t pool0, n_pool;   // its triangles in pool
    int32_t n_tris;          // triangles of its subtree in flatten order (collinear ones included)
  };
  std::vector<SharedMesh> mesh;      // placed meshes, in order of first placement
  std::vector<int32_t> place_mesh;   // per placement, in insertion order: its mesh
  std::vector<int32_t> place_slot;   // ... and its kInstance record in obj
  std::vector<Obj> pool;             // triangles in local space, inst = -1
  std::vector<int32_t> pool_j;       // pool slot -> index j in its mesh's flatten order (insertion index first(p) + j)
  std::vector<int32_t> pool_attr;    // attribute record of a pool slot or -1; empty when obj_attr is
  std::vector<Node> bnodes;          // the bottom-level BVHs, one after the other
  // Moving placements (rt_nw_move, DESIGN.md §9 "Moving placements"): how many
  // kInstance records carry a motion (aux = 1; rtmi_nw_types.h kInstance).  Each
  // has an Inst of its own at the end of inst, holding o0; its top-level box
  // is swept over the render times [0, 1].
  int32_t n_moving = 0;
  // Affine placements (rt_nw_transform, DESIGN.md §9 "Affine placements"): how
  // many kInstance records carry aux bit 1.  Each has two Inst rows of its own
  // at the end of inst, read as one AffInst (rtmi_nw_types.h).
  int32_t n_affine = 0;
};

// Flatten the world and build the BVH (RT_OK or RT_E*).
int build_device_scene(rt_nw_scene *s, DeviceScene &out);
// rt_nw_scene_instancing_stats: counts of build_device_scene, host only.
int scene_instancing_stats(rt_nw_scene *s, int32_t out[6]);
// rt_nw_scene_grid_stats: the grid of build_device_scene, host only.
int scene_grid_stats(rt_nw_scene *s, int32_t *dims3, int32_t *max_cell, int32_t *n_big, int32_t *n_refs);

// Checkpoint file of the progressive accumulator (rt_nw_accum_save / _load / _info; rtmi_nw.h): this
// header, little-endian, then the int64 sums [nrows][W][3].  The layout of the One-Weekend file
// (rtmi_device.hip) under a magic of its own.  Host only (rtmi_nw_scene.cpp).
struct CkptHeader {
  char magic[8];  // "RTMINWA1"
  int32_t W, H, row0, row_step, nrows, spp_done, max_depth, zero;
  uint64_t seed, scene_hash, camera_hash;
};
static_assert(sizeof(CkptHeader) == 64, "checkpoint header layout");
// Writes path atomically (path + ".tmp", then rename): the header with the magic filled in, then the
// W * nrows * 3 sums of raw.  RT_EIO.
int ckpt_write(const char *path, const CkptHeader &h, const int64_t *raw);
// The header of path: RT_EIO for a file that cannot be opened, is shorter than a header or starts with
// another magic.  With raw: also the body, the header's W * nrows * 3 sums — RT_EIO when W < 1 or nrows <
// 0, or when the file holds fewer or more bytes than that.
int ckpt_read(const char *path, CkptHeader &h, std::vector<int64_t> *raw);
// Checkpoint file of the adaptive accumulator (rt_nw_adapt_save / _load / _info): the same header under the magic
// "RTMINWD1" (spp_done: the largest count a pixel holds), then the int64 sums [nrows][W][3], the uint64 second
// moments [nrows][W] and the int32 counts [nrows][W].  Written and read as the progressive file is: atomically;
// RT_EIO for a file of another magic (a progressive checkpoint among them), a short one or a longer one.  The three
// vectors are filled together or not at all (all null: the header alone).
int adapt_ckpt_write(const char *path, const CkptHeader &h, const int64_t *sum, const uint64_t *m2, const int32_t *n);
int adapt_ckpt_read(const char *path, CkptHeader &h, std::vector<int64_t> *sum, std::vector<uint64_t> *m2, std::vector<int32_t> *n);
// FNV-1a 64 of the camera's bytes (the shutter included)
uint64_t camera_hash(const rt_nw_camera *cam);

// What the denoiser (rtmi_nw_denoise.hip) uses of a context, whose layout stays with rtmi_nw.hip: the device, the
// context's stream (a hipStream_t) and the filter's scratch images, one device allocation that the context's
// destructor frees.  ctx_begin / ctx_end put work on `stream` into the context's order as every launch of
// rtmi_nw.hip is (it waits for the last work on another stream, and records its own end); ctx_idle waits for
// everything the context has launched, before the scratch is replaced.
struct DenoiseScratch {
  void *p = nullptr;
  size_t pixels = 0;
};
struct CtxLink {
  int32_t device = 0;
  void *stream = nullptr;
  DenoiseScratch *scratch = nullptr;
};
int ctx_link(rt_nw_ctx *ctx, CtxLink &out);
int ctx_begin(rt_nw_ctx *ctx, void *stream);
void ctx_end(rt_nw_ctx *ctx, void *stream);
int ctx_idle(rt_nw_ctx *ctx);

}  // namespace nw
}  // namespace rtmi
