// rtmi_nw_types.h — flattened Next-Week scene records, shared by the host
// scene builder (rtmi_nw_scene.cpp) and the gfx950 kernels (rtmi_nw.hip).
// Layout and semantics: DESIGN.md §9.  Not installed.
#pragma once

#include <cstdint>

namespace rtmi {
namespace nw {

// object kinds (the leaf hittables of rt_next_week/cuda/)
enum ObjKind : int32_t {
  kSphere = 0,        // sphere.h            g0 = {c, r}
  kMovingSphere = 1,  // moving_sphere.h     g0 = {c0, r}, g1 = {c1, time0}, g2.x = time1
  kRectXY = 2,        // aarect.h xy_rect    g0 = {x0, x1, y0, y1}, g1.x = k
  kRectXZ = 3,        //          xz_rect    g0 = {x0, x1, z0, z1}, g1.x = k
  kRectYZ = 4,        //          yz_rect    g0 = {y0, y1, z0, z1}, g1.x = k
  kBox = 5,           // box.h               g0 = {p0, 0}, g1 = {p1, 0}
  kMedium = 6,        // constant_medium.h   boundary geometry as its kind (aux & 255), g2.w = -1/density,
                      //                     aux >> 8 = scattering-distance samples
  kTriangle = 7,      // triangle (two-sided, watertight): the vertices as nine floats,
                      //                     g0 = {v0, v1.x}, g1 = {v1.y, v1.z, v2.x, v2.y}, g2.x = v2.z
  kInstance = 8,      // one placement of a shared mesh (rt_nw_shared; device scene only, never in the flat
                      //                     view): g0 as int32 bits = {first bottom-level node, one past its
                      //                     last, first pool slot, first(p): the insertion index of the
                      //                     placement's triangle 0}, g1.x as int32 bits = pool slots of the mesh;
                      //                     inst = the placement's Inst or -1 (DESIGN.md §9 "Shared meshes").
                      //                     A moving placement (rt_nw_move): aux = 1, its Inst holds o0,
                      //                     g1[1..3] = o1, g2 = {time1, time0} (DevObj: t1 = time1, mat = the bits
                      //                     of time0; a static placement's are zero).
                      //                     An affine placement (rt_nw_transform): aux bit 1 (aux = 2, moving 3);
                      //                     inst = the first of two Inst rows read as one AffInst, whose off is
                      //                     o0; the motion words as above
};

// material kinds = RT_NW_* (rtmi_nw.h)
enum MatKind : int32_t { kLambertian = 0, kMetal = 1, kDielectric = 2, kDiffuseLight = 3, kIsotropic = 4 };
// texture kinds
enum TexKind : int32_t { kSolid = 0, kChecker = 1, kNoise = 2, kImage = 3 };

struct Obj {  // 64 B
  float g0[4], g1[4], g2[4];
  int32_t kind, mat, inst, aux;  // aux: medium -> boundary kind | samples << 8; other objects -> twin
                                 // medium + 1 (0: none): the medium whose boundary this object is
};
constexpr int kMaxMedia = 32;
// The device's record of a non-medium object (48 B: three float4 loads, 25%
// less LDS than Obj): media live in their own list, so only the moving
// sphere's time1 — or a triangle's ninth float, v2.z — remains of g2.
struct DevObj {
  float g0[4], g1[4];
  int32_t ka;  // kind | aux << 8 (one 32-bit field: no sub-dword loads)
  int32_t mat;
  float t1;  // moving sphere: time1; triangle: v2.z (Obj g2[0])
  int32_t inst;
};
static_assert(sizeof(DevObj) == 48, "DevObj layout");
// Per-corner attributes of a triangle built with RT_NW_MESH_SMOOTH / _UV (64 B;
// rt_nw_scene_flat_attr exposes these records as they are), in the winding
// the builder settled.  Global memory only: a triangle's record is read once
// per segment, when its hit record is made (make_rec), never by a walk.
struct TriAttr {
  float n[9];     // unit normals of v0, v1, v2 (flags bit 0)
  float uv[6];    // texture coordinates of v0, v1, v2 (flags bit 1)
  int32_t flags;  // bit 0: normals present, bit 1: uvs present
};
static_assert(sizeof(TriAttr) == 64, "TriAttr layout");
struct Inst {  // 32 B; world = translate(rotate_y(local)) (hittable.h:49-189)
  float c, s;      // cos, sin of the composed rotate_y angle
  float off[3];    // composed translation
  int32_t flags;   // bit 0 rotation present, bit 1 translation present
  int32_t pad[2];
};
// An affine placement's two Inst rows (rt_nw_transform, TRI = 5): local = m (world - off)
struct AffInst {  // 64 B
  float m[9];      // float(A^-1), row-major
  float off[3];    // float(b); a moving placement's o0
  int32_t flags;   // 4
  int32_t pad[3];
};
// The translation of a moving placement (rt_nw_move) at ray time T — the one
// place it is written, for the host's flat view (rt_nw_scene_flat_at) and the
// TRI = 4 kernels alike.  o0, o1: the placement's composed translations with
// the node at offset0 and at offset1, each rounded to float; f is
// moving_center's rule (rtmi_nw_path.h).  A subtract, a multiply and an add,
// each rounded on its own: contraction is switched off here whatever the
// command line says, so numpy float32 reproduces the value exactly.
#if defined(__HIPCC__)
#define RTMI_NW_HD __host__ __device__
#else
#define RTMI_NW_HD
#endif
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
RTMI_NW_HD inline void motion_offset(const float o0[3], const float o1[3], float time0, float time1, float T, float out[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float f = (time0 == 0.0f && time1 == 1.0f) ? T : (T - time0) / (time1 - time0);
  for (int a = 0; a < 3; ++a) {
    const float d = o1[a] - o0[a];
    const float fd = f * d;
    out[a] = o0[a] + fd;
  }
}

struct Mat {  // 16 B
  int32_t kind, tex;
  float fuzz, ir;
};
struct Tex {  // 32 B
  int32_t kind, a, b, pad;  // checker: a = even, b = odd; noise: a = perlin; image: a = image
  float rgb[3], scale;
};
struct Image {
  int32_t offset, w, h, pad;  // offset into the image byte pool; w = 0: no data (cyan)
};

constexpr int kPerlinN = 256;
constexpr int kNodeLeafMax = 4;

static_assert(sizeof(Obj) == 64, "Obj layout");
static_assert(sizeof(Inst) == 32, "Inst layout");
static_assert(sizeof(AffInst) == 2 * sizeof(Inst), "AffInst layout");

}  // namespace nw
}  // namespace rtmi
