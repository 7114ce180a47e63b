/* include/rtmi_nw.h — C ABI of librtmi's Next-Week renderer (SURVEY §8(f)
 * rank 4): the scene vocabulary of the reference's rt_next_week/cuda/ —
 * textures (texture.h, perlin.h), materials incl. emission and isotropic
 * phase (material.h), spheres and moving spheres (sphere.h, moving_sphere.h),
 * axis-aligned rectangles and boxes (aarect.h, box.h), instances
 * (translate / rotate_y, hittable.h:49-191), participating media
 * (constant_medium.h), a background colour and emission-aware path
 * integration (get_color, main.cu:47-101) — rendered by gfx950 kernels in
 * the same wave-queue / fixed-point design as the RTIOW path.
 *
 * The reference builds its scenes with `new` on the device and renders them
 * through virtual hit()/scatter() calls.  Here the caller builds a host-side
 * scene with the calls below (one per reference constructor); the library
 * flattens it — every leaf primitive carrying its composed rotate_y +
 * translate instance — builds a BVH and uploads it.
 *
 * Conventions are those of rtmi.h: RT_OK / negative RT_E* returns (builders
 * return the new handle, >= 0, or a negative RT_E*), rt_last_error(), no
 * CPU fallback, per-pixel colour SUMS with row 0 at the bottom.  Differences
 * from the reference's semantics are listed in DESIGN.md §9.
 */
#ifndef RTMI_NW_H
#define RTMI_NW_H

#include "rtmi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_nw_scene rt_nw_scene; /* host-side scene under construction */
typedef struct rt_nw_ctx rt_nw_ctx;     /* one device, its stream, the resident scene */

/* camera.h:24-83 (Next-Week camera: shutter interval [time0, time1]) */
typedef struct rt_nw_camera {
  rt_camera cam;
  double time0, time1;
} rt_nw_camera;

/* camera::camera(lookfrom, lookat, vup, vfov, aspect, aperture, focal_dist,
 * time0, time1) camera.h:24-62, evaluated in double, rounded to float on use. */
int rt_nw_camera_init(rt_nw_camera *cam, const double lookfrom[3], const double lookat[3],
                      const double vup[3], double vfov_deg, double aspect_ratio, double aperture,
                      double focus_dist, double time0, double time1);

int rt_nw_scene_create(rt_nw_scene **out);
int rt_nw_scene_destroy(rt_nw_scene *s);

/* ---- textures (texture.h) ---------------------------------------------- */
int rt_nw_tex_solid(rt_nw_scene *s, double r, double g, double b);        /* solid_color      */
int rt_nw_tex_checker(rt_nw_scene *s, int32_t even, int32_t odd);          /* checker_texture  */
/* noise_texture(scale) over a perlin table: ranvec[256*3] (xyz per entry)
 * and perm[3*256] (perm_x, perm_y, perm_z), perlin.h:8-21. */
int rt_nw_tex_noise(rt_nw_scene *s, double scale, const float *ranvec, const int32_t *perm);
/* image_texture(data, w, h) texture.h:84-124: rgb bytes, w*h*3, row 0 at the
 * top (stb_image order); copied.  data == NULL renders cyan (texture.h:96). */
int rt_nw_tex_image(rt_nw_scene *s, const uint8_t *rgb, int32_t w, int32_t h);

/* ---- materials (material.h) -------------------------------------------- */
enum { RT_NW_LAMBERTIAN = 0, RT_NW_METAL = 1, RT_NW_DIELECTRIC = 2, RT_NW_DIFFUSE_LIGHT = 3, RT_NW_ISOTROPIC = 4 };
int rt_nw_mat_lambertian(rt_nw_scene *s, int32_t tex);
int rt_nw_mat_metal(rt_nw_scene *s, int32_t tex, double fuzz); /* fuzz clamped to <= 1 (material.h:58-62) */
int rt_nw_mat_dielectric(rt_nw_scene *s, double ir);
int rt_nw_mat_diffuse_light(rt_nw_scene *s, int32_t tex);
int rt_nw_mat_isotropic(rt_nw_scene *s, int32_t tex);

/* ---- objects (handles; an object is rendered once added to the world) --- */
enum { RT_NW_XY = 0, RT_NW_XZ = 1, RT_NW_YZ = 2 };
int rt_nw_sphere(rt_nw_scene *s, const double center[3], double radius, int32_t mat);
int rt_nw_moving_sphere(rt_nw_scene *s, const double center0[3], const double center1[3], double time0,
                        double time1, double radius, int32_t mat);
/* xy_rect(a0,a1,b0,b1,k) etc. aarect.h: (a, b) are the in-plane axes in
 * order (xy: x,y; xz: x,z; yz: y,z), k the plane coordinate. */
int rt_nw_rect(rt_nw_scene *s, int32_t plane, double a0, double a1, double b0, double b1, double k, int32_t mat);
int rt_nw_box(rt_nw_scene *s, const double p0[3], const double p1[3], int32_t mat);
/* A triangle (the reference's triangles/ chapter, triangle.h), two-sided and
 * watertight (Woop, Benthin, Wald 2013): counter-clockwise
 * vertices face front — the side a dielectric is entered from — and shading
 * is flat.  RT_EINVAL: a coordinate not finite as a float, or two vertices
 * equal as floats (three collinear ones are accepted and never hit: the
 * device scene leaves such a triangle out). */
int rt_nw_triangle(rt_nw_scene *s, const double v0[3], const double v1[3], const double v2[3], int32_t mat);
/* n_tris triangles over n_verts vertices (xyz each; tri_idx: three vertex
 * indices per triangle); one handle for the set, used like rt_nw_group's.
 * normals (n_normals xyz, may be NULL) fix the winding: a triangle whose
 * cross(v1 - v0, v2 - v0) points away from the sum of its corners' normals
 * has v1 and v2 exchanged.  normal_idx (three per triangle) may be NULL:
 * the corners then take the normals of their vertex indices.  Any index out
 * of range or negative: RT_EINVAL. */
int rt_nw_mesh(rt_nw_scene *s, const double *verts, int32_t n_verts, const int32_t *tri_idx, int32_t n_tris,
               const double *normals, int32_t n_normals, const int32_t *normal_idx, int32_t mat);
/* A Wavefront OBJ file as one mesh of material `mat`; *n_tris (may be NULL)
 * its triangle count.  Read: v, vn, and f with corners a, a/t, a//n or
 * a/t/n, negative indices counting back from the latest statement; polygons
 * are fan-triangulated in the file's winding, and faces with normals get
 * rt_nw_mesh's winding fix.  Ignored: vt, o, g, s, usemtl, mtllib (no file
 * but `path` is opened), '#' comments, blank lines, CR LF endings.
 * RT_EINVAL with the line number in rt_last_error(): a malformed number or
 * index, an index out of range, a face with fewer than three corners, a
 * degenerate triangle; RT_EIO: the file cannot be opened or read. */
int rt_nw_load_obj(rt_nw_scene *s, const char *path, int32_t mat, int32_t *n_tris);
/* The scene of `rtmi_nw_render --obj` into an empty scene: the file's mesh
 * scaled uniformly and centred into [-1, 1] x [0, 2] x [-1, 1] (largest extent
 * 2 units, standing on y = 0) with material mat_kind (RT_NW_LAMBERTIAN,
 * _METAL or _DIELECTRIC), on a checker ground, under one 3 x 3 xz_rect light
 * (emission 6) at y = 5, background (0.05, 0.07, 0.12); writes the camera:
 * from (3.2, 2.4, 4.8) at the box centre (0, 1, 0), vfov 30, no aperture.
 * Errors as rt_nw_load_obj. */
int rt_nw_scene_obj_stage(rt_nw_scene *s, const char *path, int32_t mat_kind, double aspect, rt_nw_camera *cam,
                          int32_t *n_tris);
/* ---- meshes with per-corner attributes: smooth shading and texture coordinates
 * (DESIGN.md §9 "Triangles").  The calls above stay flat-shaded with the
 * barycentric u, v and never look at vt or a corner's t. */
enum { RT_NW_MESH_SMOOTH = 1, RT_NW_MESH_UV = 2, RT_NW_MESH_GEN_NORMALS = 4 };
/* rt_nw_mesh with attributes; flags == 0 and uvs == NULL: rt_nw_mesh exactly.
 * The winding is fixed from the normals as in rt_nw_mesh; when v1 and v2 are
 * exchanged, their normals and uvs go with them.
 * RT_NW_MESH_SMOOTH: a triangle all of whose corners have a normal is shaded
 *   with the normals interpolated (each normalised in double, rounded to
 *   float; how the renderer uses them: DESIGN.md §9); a triangle lacking one
 *   stays flat.  An explicit corner normal not finite as a float or of zero
 *   length: RT_EINVAL.
 * RT_NW_MESH_GEN_NORMALS (with SMOOTH): a corner without a normal (normals ==
 *   NULL here; an OBJ corner without n) takes the normalised sum, over every
 *   triangle of this call using the same vertex index, of cross(v1 - v0, v2 -
 *   v0) — in double, from the vertices as given, so area-weighted.  A
 *   triangle with a vertex whose sum is zero or not finite stays flat.
 * RT_NW_MESH_UV: uvs holds n_uvs (u, v) pairs, uv_idx three indices per
 *   triangle (NULL: the vertex indices); a triangle's texture u, v are then
 *   the interpolated pair instead of its barycentric weights, passed to the
 *   texture unwrapped (an image texture clamps to [0, 1]).  An index out of
 *   range, a value not finite as a float, or UV without uvs: RT_EINVAL. */
int rt_nw_mesh_attr(rt_nw_scene *s, const double *verts, int32_t n_verts, const int32_t *tri_idx, int32_t n_tris,
                    const double *normals, int32_t n_normals, const int32_t *normal_idx, const double *uvs,
                    int32_t n_uvs, const int32_t *uv_idx, uint32_t flags, int32_t mat);
/* rt_nw_load_obj under flags.  SMOOTH uses the file's vn (GEN_NORMALS: fills
 * in the corners without one).  UV reads `vt u [v [w]]` (v defaults to 0, w is
 * ignored) and the t of a corner (negative: counting back from the latest vt):
 * a malformed vt, or a t of 0 or out of range, is RT_EINVAL with the line
 * number; a face with a corner lacking t gets no uvs and keeps its
 * barycentric u, v.  Without UV, vt lines and t are ignored as by rt_nw_load_obj. */
int rt_nw_load_obj_attr(rt_nw_scene *s, const char *path, int32_t mat, uint32_t flags, int32_t *n_tris);
/* rt_nw_scene_obj_stage with the mesh loaded under flags; rgb (w * h * 3 bytes
 * as rt_nw_tex_image, may be NULL) becomes the texture of the mesh's
 * lambertian or metal material (with RT_NW_DIELECTRIC: RT_EINVAL). */
int rt_nw_scene_obj_stage_attr(rt_nw_scene *s, const char *path, int32_t mat_kind, uint32_t flags, const uint8_t *rgb,
                               int32_t w, int32_t h, double aspect, rt_nw_camera *cam, int32_t *n_tris);
/* rt_nw_scene_obj_stage_attr with the mesh staged copies x copies times as one
 * shared mesh (rt_nw_shared): a field on the checker ground, 3 units between
 * neighbours, centred on the origin; copy q = i * copies + k (i along x, k
 * along z) is rotate_y(37 q degrees), then translated to
 * (3 (i - (copies - 1) / 2) + 0.4 sin(1.7 q), 0, 3 (k - (copies - 1) / 2) +
 * 0.4 cos(2.3 q)); the camera keeps its line of sight and stands 0.5 + 0.75
 * copies times as far away.  copies == 1: rt_nw_scene_obj_stage_attr exactly
 * (no shared handle).  copies outside 1..256: RT_EINVAL. */
int rt_nw_scene_obj_stage_copies(rt_nw_scene *s, const char *path, int32_t mat_kind, uint32_t flags, const uint8_t *rgb,
                                 int32_t w, int32_t h, int32_t copies, double aspect, rt_nw_camera *cam, int32_t *n_tris);
/* constant_medium(boundary, density, tex) constant_medium.h: boundary is a
 * sphere, moving sphere or box object, optionally under translate/rotate_y
 * (a rectangle, a triangle, a shared handle or a set of objects:
 * RT_EUNSUPPORTED). */
/* rt_nw_scene_obj_stage_copies with every placement under rt_nw_move from (0,
 * 0, 0) to `move` over [0, 1] (`rtmi_nw_render --obj-move`); copies == 1: the
 * model as one moving placement of a shared mesh. */
int rt_nw_scene_obj_stage_moving(rt_nw_scene *s, const char *path, int32_t mat_kind, uint32_t flags, const uint8_t *rgb,
                                 int32_t w, int32_t h, int32_t copies, const double move[3], double aspect,
                                 rt_nw_camera *cam, int32_t *n_tris);
/* rt_nw_scene_obj_stage_copies with copy q of the field as an affine placement
 * (rt_nw_transform; `rtmi_nw_render --obj-tumble`): uniform scale 0.75 + 0.25
 * sin(2.9 q), turned 37 q degrees about normalize(sin 1.3 q, 1, cos 0.7 q), at
 * its field position, lifted until the lowest corner of its transformed stage
 * box stands on y = 0.  copies == 1: the model as one such placement (q = 0).
 * move, when not null: every placement under rt_nw_move as in
 * rt_nw_scene_obj_stage_moving. */
int rt_nw_scene_obj_stage_tumbled(rt_nw_scene *s, const char *path, int32_t mat_kind, uint32_t flags, const uint8_t *rgb,
                                  int32_t w, int32_t h, int32_t copies, const double *move, double aspect,
                                  rt_nw_camera *cam, int32_t *n_tris);
int rt_nw_constant_medium(rt_nw_scene *s, int32_t boundary, double density, int32_t tex);
/* Scattering-distance samples of a medium per ray segment (1..8, default 1):
 * each draws -log(u)/density anew and the last one that lands inside the
 * boundary wins — what the reference's bvh_node does to a medium alone in a
 * span-1 leaf, which it evaluates twice (bvh.h:90-97, 147-151).
 * Media are resolved before the other objects of a segment, and a medium's
 * hit hides its own boundary object when that is in the world too (the
 * reference visits constant_medium after its boundary, main.cu:386-391, and
 * constant_medium::hit ignores t_max).  DESIGN.md §9. */
int rt_nw_medium_samples(rt_nw_scene *s, int32_t medium, int32_t samples);
/* hittable_list / bvh_node of objects (one handle for the set). */
int rt_nw_group(rt_nw_scene *s, const int32_t *objects, int32_t n);
int rt_nw_translate(rt_nw_scene *s, int32_t object, const double offset[3]); /* hittable.h:49-88  */
int rt_nw_rotate_y(rt_nw_scene *s, int32_t object, double angle_deg);       /* hittable.h:90-189 */
/* `object` as shared geometry: a new handle, used like any object handle (in
 * rt_nw_group, rt_nw_translate, rt_nw_rotate_y, rt_nw_world_add) any number of
 * times; every occurrence reached from the world is one placement.  The scene
 * renders exactly — bit for bit — as if `object` itself stood at every
 * occurrence, and rt_nw_scene_flat / _flat_attr return that expansion
 * (insertion order and `inst` table included: placement p's triangle j, in the
 * subtree's flatten order, has insertion index first(p) + j).  The device
 * holds the triangles once, under a bottom-level BVH of their own, and one
 * small record per placement (DESIGN.md §9 "Shared meshes"); a scene with a
 * placement has no uniform grid and renders with the BVH.
 * The subtree of `object` may hold only triangles and groups of them (the
 * handles of rt_nw_triangle, rt_nw_mesh, rt_nw_mesh_attr, rt_nw_load_obj* and
 * rt_nw_group over those): anything else under it — another primitive kind,
 * a translate or rotate node, a medium, another shared handle — is
 * RT_EUNSUPPORTED; no triangle under it: RT_EINVAL. */
int rt_nw_shared(rt_nw_scene *s, int32_t object);
/* A translate node whose offset is linear in the ray's time, like
 * moving_sphere's centre: offset0 at time0, offset1 at time1, extrapolated
 * outside that interval (camera shutters lie in [0, 1]).  A new handle, used
 * like rt_nw_translate's.  Only a placement of a shared mesh can move: the
 * subtree of `object` must be one rt_nw_shared handle, optionally under
 * rt_nw_translate / rt_nw_rotate_y nodes — a primitive, a group, a medium, a
 * flattened mesh, or another rt_nw_move above or below: RT_EUNSUPPORTED; as a
 * medium's boundary: RT_EUNSUPPORTED.  time0 == time1, a time not finite or an
 * offset not finite as a float: RT_EINVAL.  offset0 == offset1 is legal.
 * The translation at ray time T (DESIGN.md §9 "Moving placements"): o0 and o1
 * are the placement's composed translations with the node at offset0 and at
 * offset1, each composed in double as a static rt_nw_translate's and rounded to
 * float; f = T when (time0, time1) == (0, 1), else (T - time0) / (time1 -
 * time0); off(T) = o0 + f * (o1 - o0), every operation a float operation
 * rounded on its own.  The image at the instant T (shutter [T, T]) is that of
 * the static scene rt_nw_scene_flat_at(T) describes, bit for bit. */
int rt_nw_move(rt_nw_scene *s, int32_t object, const double offset0[3], const double offset1[3], double time0,
               double time1);
/* A placement node with a general affine map, world = A local + b.  m is
 * row-major 3x4: A = {m[0..2], m[4..6], m[8..10]}, b = {m[3], m[7], m[11]}.  A
 * new handle, used like rt_nw_translate's.  Only a placement of a shared mesh
 * takes an affine map: the subtree of `object` must be one rt_nw_shared handle
 * under any chain of rt_nw_translate, rt_nw_rotate_y, rt_nw_transform and at
 * most one rt_nw_move node, in any order — a primitive, a group, a medium, a
 * flattened mesh: RT_EUNSUPPORTED; as a medium's boundary, or under
 * rt_nw_shared: RT_EUNSUPPORTED.  RT_EINVAL at the call: an entry not finite
 * as a float; det(A) <= 0 (a singular map, or a mirror: out of scope);
 * |A|_F |A^-1|_F > 1024 (Frobenius norms; every matrix whose singular values
 * lie in [1/16, 16] passes).  The same bound holds for a placement's composite
 * map and is checked wherever the scene is flattened (rt_nw_scene_flat*, the
 * stats calls, rt_nw_ctx_set_scene): RT_EINVAL naming the placement.
 * Composition runs in double from the world down, (A, b) starting at (I, 0):
 * translate(off): b += A off; rotate_y: A = A Ry; transform(m): b += A m_b,
 * then A = A m_A; a move carries b and b1 side by side.  The kernels take the
 * world ray into the placement's frame with float(A^-1) and do not renormalise
 * the direction, so t is the world ray's (DESIGN.md §9 "Affine placements").
 * A placement whose chain holds no transform node is built exactly as before.
 * In the flat view an affine placement's triangles appear BAKED: vertices
 * float(A v + b(T)) from the double vertices, inst = -1, attribute normals
 * normalize(A^-T n) computed in double and rounded, insertion indices first(p)
 * + j as always.  For affine placements the flat view is therefore the nearest
 * static scene, NOT a bit-for-bit expansion: transforming the ray and
 * transforming the vertices round differently. */
int rt_nw_transform(rt_nw_scene *s, int32_t object, const double m[12]);
int rt_nw_world_add(rt_nw_scene *s, int32_t object);
int rt_nw_set_background(rt_nw_scene *s, double r, double g, double b);

/* The reference's scenes, create_world main.cu:415-490 (`which` = its switch
 * case: 1 random_scene, 2 two_spheres, 3 two_perlin_spheres, 4 earth,
 * 5 simple_light, 6 cornell_box, 7 cornell_smoke, 8 rt_next_week_final_scene).
 * Random draws come from a restatement of curand XORWOW seeded as the
 * reference seeds it (curand_init(1984, 0, 0), main.cu:103-107).  `image`
 * (w*h*3 bytes, may be NULL) is the earth texture.  Writes the camera the
 * reference uses for that scene at `aspect` (main.cu:486-489).  flags bit 0:
 * evaluate the three draws of vec3(rnd, rnd, rnd) right to left (argument
 * evaluation order is unspecified in C++; default left to right). */
enum { RT_NW_ARGS_RTL = 1 };
int rt_nw_scene_preset(rt_nw_scene *s, int32_t which, const uint8_t *image, int32_t w, int32_t h,
                       double aspect, uint32_t flags, rt_nw_camera *cam);

/* curand XORWOW restated (curand_init(seed, 0, 0) then curand_uniform):
 * n uniforms in (0, 1].  Validation of the scene generator. */
int rt_nw_xorwow_uniforms(uint64_t seed, int32_t n, float *out);

/* Flattened view of a scene (what the device renders), for tests and the
 * oracle.  Pointers stay valid until the scene is modified or destroyed.
 *   obj  : n_obj * 16 floats: g0[4] g1[4] g2[4] then kind, mat, inst, aux as
 *          int32 bit patterns (layout: DESIGN.md §9; aux: medium -> boundary
 *          kind | samples << 8, other -> insertion index of the medium whose
 *          boundary it is + 1, or 0).  A triangle (kind 7) stores its
 *          vertices as nine floats: g0 = {v0.xyz, v1.x}, g1 = {v1.y, v1.z,
 *          v2.x, v2.y}, g2[0] = v2.z, in the winding the builder settled.
 *   inst : n_inst * 8 floats: cos, sin, off.x, off.y, off.z, flags(int bits), 0, 0
 *   mat  : n_mat * 4: kind(int bits), tex(int bits), fuzz, ir
 *   tex  : n_tex * 8: kind, a, b, 0 (int bits), r, g, b, scale
 *   perlin_vec : n_perlin * 256 * 4 floats; perlin_perm : n_perlin * 768 int32
 *   image_px : all image bytes; image_desc : n_image * 4 int32 (offset, w, h, 0) */
typedef struct rt_nw_flat {
  int32_t n_obj, n_inst, n_mat, n_tex, n_perlin, n_image;
  const float *obj, *inst, *mat, *tex, *perlin_vec;
  const int32_t *perlin_perm, *image_desc;
  const uint8_t *image_px;
  int64_t image_bytes;
  float background[3];
} rt_nw_flat;
int rt_nw_scene_flat(rt_nw_scene *s, rt_nw_flat *out); /* = rt_nw_scene_flat_at(s, 0.0, out) */
/* The flat view with every moving placement (rt_nw_move) expanded at the
 * instant float(time): its `inst` rows hold off(float(time)) with the
 * translation flag set; everything else as rt_nw_scene_flat, and the same
 * bytes at any time for a scene without a move node.  Pointers stay valid
 * until the scene is modified or a flat view at another time is taken;
 * rt_nw_scene_flat_attr follows the last flat view taken. */
int rt_nw_scene_flat_at(rt_nw_scene *s, double time, rt_nw_flat *out);
/* The triangle attribute records beside rt_nw_scene_flat (same lifetime):
 *   attr        : n_attr * 16 floats: the unit normals of v0, v1, v2 (9), their
 *                 uvs (6), flags as int32 bits (bit 0 normals, bit 1 uvs; the
 *                 absent part is zero)
 *   attr_of_obj : per flattened object its record index, or -1 */
int rt_nw_scene_flat_attr(rt_nw_scene *s, int32_t *n_attr, const float **attr, const int32_t **attr_of_obj);
/* Host only (no device needed): the uniform grid rt_nw_ctx_set_scene would
 * build for this scene — cells per axis (zeros: no grid),
 * the fullest cell's object count, the brute-force list's length and the
 * total cell references.  Any output may be null. */
int rt_nw_scene_grid_stats(rt_nw_scene *s, int32_t *dims3, int32_t *max_cell, int32_t *n_big, int32_t *n_refs);
/* Host only: what rt_nw_ctx_set_scene would build of the scene's shared meshes
 * (rt_nw_shared) — {shared meshes that are placed, placements, triangles in
 * the shared pools (each mesh once, collinear triangles left out), bottom-level
 * BVH nodes in total, top-level leaf records (objects outside placements + one
 * per placement), top-level BVH nodes}.  Without a placement the first four
 * are zero. */
int rt_nw_scene_instancing_stats(rt_nw_scene *s, int32_t out[6]);
/* Host only: {affine placements (a rt_nw_transform in their chain) reached from
 * the world, other placements}. */
int rt_nw_scene_affine_stats(rt_nw_scene *s, int32_t out[2]);
/* Host only: {moving placements (under a rt_nw_move) reached from the world,
 * static placements}. */
int rt_nw_scene_motion_stats(rt_nw_scene *s, int32_t out[2]);

/* ---- device ------------------------------------------------------------ */
int rt_nw_ctx_create(int32_t device, rt_nw_ctx **out);
int rt_nw_ctx_destroy(rt_nw_ctx *ctx);
/* Flatten, build the BVH, upload.  Synchronous. */
int rt_nw_ctx_set_scene(rt_nw_ctx *ctx, rt_nw_scene *s);
/* n_prims, n_nodes of the resident BVH.  In a scene with placements of shared
 * meshes these are the top level's: its leaf records (one per placement and
 * per object outside placements, plus the media) and its nodes; the pools and
 * bottom-level nodes are counted by rt_nw_scene_instancing_stats. */
int rt_nw_ctx_info(rt_nw_ctx *ctx, int32_t *n_prims, int32_t *n_nodes);
/* Closest-hit structure over the non-media objects (media are always tested
 * first).  RT_NW_ACCEL_BVH: the SAH BVH (skip-link walk).
 * RT_NW_ACCEL_GRID: a uniform grid walked by a 3D DDA, objects much larger
 * than the median in a brute-force list beside it; offered
 * when the scene has one (rt_nw_ctx_accel_info).  RT_NW_ACCEL_AUTO (a new
 * context's setting): the grid when it is balanced (at most 24 objects in
 * any cell), else the BVH.  All give the same closest hit, so the same image
 * bit for bit.  Replaces the choice of hittable in main.cu:420-490 (the
 * reference always wraps the world in its bvh_node). */
enum { RT_NW_ACCEL_AUTO = 0, RT_NW_ACCEL_BVH = 1, RT_NW_ACCEL_GRID = 2 };
int rt_nw_ctx_set_accel(rt_nw_ctx *ctx, int32_t accel);
/* The structure renders use now (RT_NW_ACCEL_BVH or _GRID, after AUTO is
 * resolved); the grid's cells per axis (dims3, 0 when the scene has no grid),
 * its largest cell's object count and the brute-force list's length.  Any
 * output may be null. */
int rt_nw_ctx_accel_info(rt_nw_ctx *ctx, int32_t *accel_used, int32_t *dims3, int32_t *max_cell, int32_t *n_big);
/* The whole image (main.cu:125-145 + the caller's output loop), host sums,
 * synchronous.  Pixel (i, j) samples u = (i + r)/W, v = (j + r)/H
 * (main.cu:139-140). */
int rt_nw_render(rt_nw_ctx *ctx, const rt_nw_camera *cam, int32_t W, int32_t H, int32_t spp, int32_t max_depth,
                 uint64_t seed, float *sum);
/* Rows row0 + r*row_step, r < nrows, into a DEVICE strip (as rt_render_rows). */
int rt_nw_render_rows(rt_nw_ctx *ctx, const rt_nw_camera *cam, int32_t W, int32_t H, int32_t spp,
                      int32_t max_depth, uint64_t seed, int32_t row0, int32_t row_step, int32_t nrows,
                      float *dev_strip, void *stream);
/* Progressive accumulation (resumable; as rtmi.h's rt_accum_*).  The context
 * keeps a fixed-point accumulator for a W x nrows strip (the rows of
 * rt_nw_render_rows' row set; nrows = H, row0 0, row_step 1 for a whole image),
 * an allocation of its own that a plain rt_nw_render / rt_nw_render_rows in
 * between does not touch.  rt_nw_render_pass adds samples [s_begin, s_begin +
 * s_count) of every pixel, asynchronously on `stream`, with the kernel shape
 * rt_nw_render_rows would choose; any split of [0, S) into passes, in any
 * order, gives bit for bit the sums of one rt_nw_render(..., spp = S, ...) on
 * the same rows, under any kernel shape, accelerator or RTMI_NW_CHUNK.
 * rt_nw_ctx_last_segments after a pass is that pass's count; the counts of a
 * split add up to the single render's.
 * rt_nw_render_pass validates as rt_nw_render_rows does and also refuses
 * (RT_EINVAL) s_begin < 0, s_count < 0, s_begin + s_count > 2^24 (the RNG key
 * gives a sample 24 bits, and the accumulator holds 2^24 samples of at most
 * 64.0 without overflow) and an accumulator of another W x nrows
 * (rt_nw_accum_reset).  s_count == 0 succeeds and does nothing.  Rows past H
 * stay zero.
 * rt_nw_accum_resolve converts the sums to floats into a DEVICE strip and/or a
 * HOST buffer (W*nrows*3; with a host buffer it waits); on another stream it
 * first waits for the last pass.  The accumulator is unchanged: more passes
 * may follow.  rt_nw_accum_export / rt_nw_accum_import copy the raw int64
 * accumulator (n = W*nrows*3) and its sample count out / in. */
int rt_nw_accum_reset(rt_nw_ctx *ctx, int32_t W, int32_t nrows);
int rt_nw_render_pass(rt_nw_ctx *ctx, const rt_nw_camera *cam, int32_t W, int32_t H, int32_t s_begin, int32_t s_count,
                      int32_t max_depth, uint64_t seed, int32_t row0, int32_t row_step, int32_t nrows, void *stream);
int rt_nw_accum_resolve(rt_nw_ctx *ctx, float *dev_sum, float *host_sum, void *stream);
int rt_nw_accum_export(rt_nw_ctx *ctx, int64_t *host, size_t n, int32_t *spp_done);
int rt_nw_accum_import(rt_nw_ctx *ctx, const int64_t *host, size_t n, int32_t spp_done);
/* Checkpoint files: the accumulator plus what it was rendered from.  Little
 * endian: a 64-byte header — the magic "RTMINWA1" (its digit is the version of
 * the scene serialisation below); int32 W, H, row0, row_step, nrows, spp_done,
 * max_depth, 0; uint64 seed, rt_nw_scene_hash of the scene, FNV-1a 64 of the
 * rt_nw_camera's bytes (the shutter included) — then the int64 sums
 * [nrows][W][3].  rt_nw_accum_save writes atomically (path + ".tmp", then
 * rename).  rt_nw_accum_load resets the accumulator to W x nrows, fills it and
 * sets *spp_done; RT_EINVAL ("made for another render") when size, rows,
 * depth, seed, scene hash or camera hash differ; RT_EIO for a file that is
 * missing, truncated, longer than its header states or of another magic (a
 * One-Weekend checkpoint among them).  rt_nw_accum_info (host only) reads the
 * header alone: out8 = the eight int32 in file order, out3 = {seed, scene
 * hash, camera hash}. */
int rt_nw_accum_save(rt_nw_ctx *ctx, const char *path, rt_nw_scene *scene, const rt_nw_camera *cam, int32_t H, int32_t row0,
                     int32_t row_step, int32_t max_depth, uint64_t seed);
int rt_nw_accum_load(rt_nw_ctx *ctx, const char *path, rt_nw_scene *scene, const rt_nw_camera *cam, int32_t W, int32_t H,
                     int32_t row0, int32_t row_step, int32_t nrows, int32_t max_depth, uint64_t seed, int32_t *spp_done);
int rt_nw_accum_info(const char *path, int32_t out8[8], uint64_t out3[3]);
/* Adaptive sampling (DESIGN.md §9 "Adaptive sampling").  A third accumulator of
 * the context, allocations of its own that plain renders and progressive
 * passes in between do not touch.  For a W x nrows strip it holds
 *   sum  int64  [nrows][W][3]  the colour sums, as the pass accumulator's;
 *   m2   uint64 [nrows][W]     the sum over the pixel's samples of l^2, where
 *                              l = (fx + fy + fz) >> 18 and fx, fy, fz are the
 *                              sample's three 2^-32 fixed-point values: the
 *                              channel sum in units of 2^-14, below 2^22;
 *   n    int32  [nrows][W]     the samples the pixel holds.
 * A pixel holds at most RT_NW_ADAPT_MAX_SPP = 2^20 samples: a sample's l is at
 * most 192 * 2^14, and 192^2 * 2^28 * 2^20 < 2^64, so m2 cannot overflow.
 * rt_nw_adapt_reset allocates and zeroes the accumulator.
 * rt_nw_adapt_pass gives every active pixel p the samples [n[p], n[p] +
 * s_count).  `active` is a HOST array of W * nrows bytes, nonzero = sample this
 * pixel; NULL = every pixel (pixels of rows past H are never sampled).  It
 * validates as rt_nw_render_pass does and also refuses (RT_EINVAL) s_count < 0,
 * an accumulator of another W x nrows and a pass that would take an active
 * pixel past 2^20 samples (nothing is then changed).  An all-zero mask or
 * s_count == 0 succeeds, launches nothing, and rt_nw_ctx_last_segments is 0.
 * The pass is asynchronous on `stream`: its tile list is uploaded in stream
 * order into one of two device lists, so the host waits only for the pass
 * before the last one, which used that list.
 * Contract: after any sequence of passes with any masks, pixel p's sum equals
 * the pass accumulator's raw int64 sums at p after rt_nw_render_pass(s_begin =
 * 0, s_count = n[p]), bit for bit, under any kernel shape, accelerator, staging
 * path or RTMI_NW_CHUNK; m2[p] is the sum over s < n[p] of l_s^2.  An
 * all-active pass counts the segments of that rt_nw_render_pass.
 * rt_nw_adapt_export / _import copy (sum, m2, n) out / in (npix = W * nrows;
 * import refuses a count outside [0, 2^20]).  rt_nw_adapt_resolve writes the
 * per-pixel MEANS float(double(sum) * 2^-32 / n), 0 where n = 0 (sums mean
 * nothing with unequal counts), into a DEVICE strip and/or a HOST buffer
 * (W*nrows*3), as rt_nw_accum_resolve does. */
#define RT_NW_ADAPT_MAX_SPP (1 << 20)
int rt_nw_adapt_reset(rt_nw_ctx *ctx, int32_t W, int32_t nrows);
int rt_nw_adapt_pass(rt_nw_ctx *ctx, const rt_nw_camera *cam, int32_t W, int32_t H, int32_t s_count, int32_t max_depth,
                     uint64_t seed, int32_t row0, int32_t row_step, int32_t nrows, const uint8_t *active, void *stream);
int rt_nw_adapt_export(rt_nw_ctx *ctx, int64_t *sum, uint64_t *m2, int32_t *n, size_t npix);
int rt_nw_adapt_import(rt_nw_ctx *ctx, const int64_t *sum, const uint64_t *m2, const int32_t *n, size_t npix);
int rt_nw_adapt_resolve(rt_nw_ctx *ctx, float *dev_mean, float *host_mean, void *stream);
/* Host only, pure (no device): which pixels need more samples.  Per pixel, in
 * float64, in this order, without contraction:
 *   mean = (Sx + Sy + Sz) * 2^-32 / n        (the integer channel sum, exact)
 *   ex2  = m2 * 2^-28 / n
 *   var  = max(0, ex2 - mean * mean) * n / (n - 1)
 *   err  = sqrt(var / n) / max(mean, floor)
 * and err = +inf where n < 2.  A pixel is active when n < max(min_spp, 2), or
 * when err > threshold and n < max_spp.  A threshold of exactly 0 cannot be
 * met, not even by a pixel whose samples are all equal (err = 0, as of a pixel
 * that sees the background alone): every pixel below max_spp is then active,
 * and the driver's result is the plain render of max_spp samples.  For any
 * threshold above 0 such a pixel stops at min_spp; so does a pixel whose first
 * min_spp samples all missed a small light, which is why min_spp must not be
 * too small for the scene.  The mask is then dilated by `dilate`
 * pixels (a square window; 1 is the drivers' default), never onto a pixel at
 * max_spp.  err is the relative standard error of the pixel's mean channel sum;
 * below `floor` (a channel-sum level; the drivers' default 0.03: a mean of
 * 0.01 per channel, level 25 of 255 after the square-root transfer) the error
 * is judged absolutely, in units of floor, so that near-black pixels do not ask
 * for samples for ever.  m2 is quantised (l drops 18 bits) while the mean is
 * exact: l^2 is low by less than 2 l units of 2^-28 per sample, so ex2 is low
 * by less than 2^-13 * mean and err^2 by less than 2^-13 / ((n - 1) *
 * max(mean, floor)), under 0.0041 / (n - 1) at the default floor (DESIGN.md
 * §9).  active (W * nrows bytes) is required, err (W *
 * nrows doubles) and n_active may be null.  RT_EINVAL unless 0 <= min_spp <=
 * max_spp, 2 <= max_spp <= 2^20, threshold >= 0, floor > 0, dilate >= 0. */
int rt_nw_adapt_criterion(const int64_t *sum, const uint64_t *m2, const int32_t *n, int32_t W, int32_t nrows, int32_t min_spp,
                          int32_t max_spp, double threshold, double floor, int32_t dilate, uint8_t *active, double *err,
                          int64_t *n_active);
/* The driver: a whole W x H image sampled until no pixel is active.  Loop:
 * export, criterion, and a pass of min(pass_spp, max_spp - the largest active
 * count) samples over the active pixels, so no pixel passes max_spp; it ends
 * when nothing is active or, with time_limit >= 0 (seconds; < 0: none), once
 * that much time has passed since the first pass began (one pass always runs).
 * checkpoint (may be null; needs `scene`): resumed from when the file exists,
 * saved after every pass.  Outputs, each may be null: mean_out W*H*3 floats
 * (rt_nw_adapt_resolve), n_out W*H counts, err_out W*H doubles (the final
 * criterion's), stats.  on_pass (may be null) is called after every pass, and
 * after its checkpoint is saved, with `user`, the pass number from 1 and the
 * pixels that pass sampled; a nonzero return ends the run there (stopped = 2)
 * with the outputs of the samples so far.  The result depends on the arguments alone: an
 * interrupted and resumed run equals the uninterrupted one. */
typedef struct rt_nw_adapt_stats {
  int32_t passes;         /* passes this call ran */
  int32_t stopped;        /* 0: nothing was active any more; 1: the time limit; 2: on_pass returned nonzero */
  int64_t total_samples;  /* sum of n over the image */
  int64_t pixels_at_max;  /* pixels with n >= max_spp */
  int64_t samples;        /* samples this call rendered (less than total_samples after a resume) */
  int64_t segments;       /* world.hit calls of this call's passes */
  int64_t *active;        /* in: caller's array or null; out: active pixels of pass k, k < cap */
  int32_t cap, pad;
} rt_nw_adapt_stats;
typedef int (*rt_nw_adapt_on_pass)(void *user, int32_t pass, int64_t active);
int rt_nw_render_adaptive(rt_nw_ctx *ctx, rt_nw_scene *scene, const rt_nw_camera *cam, int32_t W, int32_t H, int32_t min_spp,
                          int32_t max_spp, int32_t pass_spp, double threshold, double floor, int32_t dilate, int32_t max_depth,
                          uint64_t seed, const char *checkpoint, double time_limit, float *mean_out, int32_t *n_out,
                          double *err_out, rt_nw_adapt_stats *stats, rt_nw_adapt_on_pass on_pass, void *user);
/* Checkpoints of the adaptive accumulator: the progressive file's 64-byte
 * header under the magic "RTMINWD1" (its spp_done field: the largest count a
 * pixel holds), then sum, m2 and n as laid out above.  Refusals and the atomic
 * write as rt_nw_accum_save / _load: RT_EINVAL ("made for another render"),
 * RT_EIO for a missing, truncated or overlong file or another magic — a
 * progressive checkpoint is refused here and an adaptive one by
 * rt_nw_accum_load.  rt_nw_adapt_info (host only): the header as
 * rt_nw_accum_info gives it, after checking the file's length. */
int rt_nw_adapt_save(rt_nw_ctx *ctx, const char *path, rt_nw_scene *scene, const rt_nw_camera *cam, int32_t H, int32_t row0,
                     int32_t row_step, int32_t max_depth, uint64_t seed);
int rt_nw_adapt_load(rt_nw_ctx *ctx, const char *path, rt_nw_scene *scene, const rt_nw_camera *cam, int32_t W, int32_t H,
                     int32_t row0, int32_t row_step, int32_t nrows, int32_t max_depth, uint64_t seed);
int rt_nw_adapt_info(const char *path, int32_t out8[8], uint64_t out3[3]);
/* ---- Denoising (DESIGN.md §9 "Denoising") --------------------------------
 * First-hit feature buffers, a variance guide from the adaptive accumulator
 * and an edge-avoiding a-trous wavelet filter.  Nothing here changes a render.
 *
 * rt_nw_render_features: per pixel, the mean over samples s = 0 .. fspp - 1 of
 * what the camera ray of sample (i, j, s) meets — segment 0 of
 * rt_nw_debug_trace(i, j, s), draw for draw, through the walk a render of the
 * context uses.  8 floats per pixel at (j * W + i) * 8, row 0 at the bottom:
 *   a.rgb  albedo: the background for a miss, (1, 1, 1) for a dielectric, else
 *          the texture value of the hit's material (lights and media included);
 *   n.xyz  the hit record's normal (world space, not flipped); a miss or a
 *          medium contributes (0, 0, 0), so the mean is NOT a unit vector;
 *   z      the mean ray parameter t over the samples that hit (0: none did);
 *   cov    hits / fspp (media count as hits).
 * Sums are int64 fixed point at 2^-32 per thread (albedo clamped to [0, 64],
 * normals to [-64, 64] and truncated toward zero, t to [0, 2^20]; NaN -> 0);
 * a and n are float(double(sum) * 2^-32 / fspp), z float(double(sum_t) * 2^-32
 * / hits), cov float(double(hits) / fspp).  Either of dev_feat (DEVICE, async
 * on `stream`) and host_feat (HOST, synchronous) may be null, not both, as
 * rt_nw_accum_resolve.  Validates as rt_nw_render; RT_EINVAL also for fspp
 * outside 1..1024 and for W * H >= 2^31. */
int rt_nw_render_features(rt_nw_ctx *ctx, const rt_nw_camera *cam, int32_t W, int32_t H, int32_t fspp, uint64_t seed,
                          float *dev_feat, float *host_feat, void *stream);
/* Host only, pure: the variance of each pixel's mean channel sum r + g + b,
 * from the moments of rt_nw_adapt_criterion in the same float64 order:
 *   var = float(max(0, ex2 - mean * mean) / (n - 1)),
 * which is (err * max(mean, floor))^2 of the criterion; +inf where n < 2. */
int rt_nw_adapt_variance(const int64_t *sum, const uint64_t *m2, const int32_t *n, int32_t W, int32_t nrows, float *var);
/* The filter.  Inputs (row-major, any row order as long as all agree):
 * color W*H*3 per-pixel means; var W*H, the variance of the pixel's mean
 * channel sum, or null (no luminance term); feat W*H*8 as above.
 *   prepare: A = max(a, 0.01) per channel (1 without DEMODULATE), Abar = (A.r +
 *     A.g + A.b) / 3; c' = c / A, v' = var / Abar^2; gz = max(|gx|, |gy|), the
 *     central difference of z over the in-image neighbours with cov > 0 (one
 *     missing: the one-sided difference to the pixel itself; both: 0).
 *   pass k = 0 .. iterations - 1, step = 2^k: taps (dx, dy) in {-2..2}^2 at
 *     offset step * (dx, dy), those outside the image skipped; h = (1/16, 1/4,
 *     3/8, 1/4, 1/16);
 *       w = h(dx) h(dy) exp(-(sigma_n / 2) |n_p - n_q|^2
 *                           - |z_p - z_q| / (sigma_z gz_p step max(|dx|, |dy|) + 1e-3 |z_p| + 1e-12)
 *                           - |l_p - l_q| / (sigma_l sqrt(vt_p) + 1e-6)),
 *     l the channel sum of c', vt_p the 3x3 binomial mean of the pass's input
 *     v' around p over the in-image pixels whose v' is finite.  The luminance
 *     term is absent without var and for a centre whose v' is not finite (a
 *     pixel of fewer than two samples).  The centre tap has w = 9/64.  A tap
 *     whose colour, v' or weight is not finite is skipped; a centre whose
 *     colour is not finite passes through unchanged.
 *       c'_out = sum w c'_q / sum w,  v'_out = sum w^2 v'_q / (sum w)^2
 *     (v'_out = v'_p where that is not finite).
 *   finish: out = c' A, var_out = v' Abar^2.
 * RT_NW_DENOISE_NO_EDGES sets every edge weight to 1: the plain B3 blur, a
 * test instrument.  The scratch images belong to the context (52 bytes per
 * pixel, grown on demand, freed by rt_nw_ctx_destroy).  rt_nw_denoise takes
 * DEVICE arrays and is asynchronous on `stream` (null: the context's);
 * dev_out may be dev_color.  rt_nw_denoise_host takes HOST arrays and is
 * synchronous.  p null: the defaults.  RT_EINVAL: iterations outside 1..8, a
 * sigma that is not finite or <= 0, unknown flag bits, W or H < 1, a null
 * color, feat or out.  rt_nw_denoise_params_default / _check are host only. */
#define RT_NW_DENOISE_DEMODULATE 1u
#define RT_NW_DENOISE_NO_EDGES 2u
typedef struct rt_nw_denoise_params {
  int32_t iterations; /* 1..8, default 5 */
  float sigma_l;      /* default 4 */
  float sigma_n;      /* default 128 */
  float sigma_z;      /* default 1 */
  uint32_t flags;     /* default RT_NW_DENOISE_DEMODULATE */
} rt_nw_denoise_params;
int rt_nw_denoise_params_default(rt_nw_denoise_params *p);
int rt_nw_denoise_params_check(const rt_nw_denoise_params *p);
int rt_nw_denoise(rt_nw_ctx *ctx, int32_t W, int32_t H, const float *dev_color, const float *dev_var, const float *dev_feat,
                  const rt_nw_denoise_params *p, float *dev_out, float *dev_var_out, void *stream);
int rt_nw_denoise_host(rt_nw_ctx *ctx, int32_t W, int32_t H, const float *color, const float *var, const float *feat,
                       const rt_nw_denoise_params *p, float *out, float *var_out);
/* The driver: rt_nw_render_adaptive with the same arguments (threshold 0: the
 * plain render of max_spp), then rt_nw_render_features (fspp samples, `seed`),
 * rt_nw_adapt_variance of the accumulator and rt_nw_denoise, on the context's
 * stream.  denoised_out: W*H*3 floats, required.  The other outputs are those
 * of rt_nw_render_adaptive, bit for bit.  The variance is formed on the host,
 * as the driver's criterion is: after the render the accumulator is exported
 * (36 B per pixel), the variance uploaded (4 B per pixel) and a device buffer
 * of 48 B per pixel allocated for the call and freed after it; none of that
 * is in the kernel times of profiles/denoise/README.md. */
int rt_nw_render_denoised(rt_nw_ctx *ctx, rt_nw_scene *scene, const rt_nw_camera *cam, int32_t W, int32_t H, int32_t min_spp,
                          int32_t max_spp, int32_t pass_spp, double threshold, double floor, int32_t dilate, int32_t max_depth,
                          uint64_t seed, const char *checkpoint, double time_limit, float *mean_out, int32_t *n_out,
                          double *err_out, rt_nw_adapt_stats *stats, rt_nw_adapt_on_pass on_pass, void *user, int32_t fspp,
                          const rt_nw_denoise_params *p, float *denoised_out);
/* Host only (no device needed): FNV-1a 64 over everything of the scene that
 * can change a pixel, and nothing else — no address, not the accelerator
 * setting, no BVH or grid.  The same value in any process that builds the
 * scene with the same calls.  Serialisation (every number in its in-memory
 * little-endian form; "table" = the record count as int64, then the records):
 *   the bytes "RTMINWS1";
 *   of the flat view at time 0 (rt_nw_scene_flat, rt_nw_flat's layouts): the
 *     tables obj (16 words each, aux included: medium samples, twins), inst,
 *     mat, tex, perlin_vec (floats), perlin_perm (int32), image_desc,
 *     image_px (bytes); the three background floats;
 *   the tables of the attribute records (16 words each, creation order) and of
 *     the locator (one int32 per flattened object: its record or -1);
 *   the placement count as int64, then per placement reached from the world,
 *     in insertion order: int32 first, count, flags (1 moving | 2 affine);
 *     moving: floats o0[3], o1[3], time0, time1 (rt_nw_move's composed ends);
 *     affine: floats M[9] = float(A^-1) row-major and off[3] = float(b), the
 *     rows the kernels read (the flat view only shows them baked).
 * Taking the hash takes the flat view at time 0 and puts a view the caller
 * held at another time back (its pointers are to be fetched again). */
int rt_nw_scene_hash(rt_nw_scene *s, uint64_t *out);
/* Debug (parity investigations): the path segments of ONE camera sample
 * (pixel i, j, sample s), up to cap: per segment 12 floats o.xyz, d.xyz, t,
 * the winner's insertion index (int32 bits, -1: miss), its hit-record normal
 * xyz and the box face (int32 bits, -1: none).  *n = segments. */
int rt_nw_debug_trace(rt_nw_ctx *ctx, const rt_nw_camera *cam, int32_t W, int32_t H, int32_t max_depth,
                      uint64_t seed, int32_t i, int32_t j, int32_t s, float *rec, int32_t cap, int32_t *n);
/* rt_nw_debug_trace, and *time: the traced sample's ray time. */
int rt_nw_debug_trace_t(rt_nw_ctx *ctx, const rt_nw_camera *cam, int32_t W, int32_t H, int32_t max_depth,
                        uint64_t seed, int32_t i, int32_t j, int32_t s, float *rec, int32_t cap, int32_t *n, float *time);
/* Validation: the closest hit of n given rays through the walk a render of
 * this context uses (the uniform grid or the BVH: rt_nw_ctx_accel_info) —
 * rays {o.xyz, d.xyz, time, unused} per ray (8 floats), keys the segments'
 * medium keys (null: 0).  Out: the winner's insertion index (-1: miss), t
 * and the box face (-1: none), as one segment of rt_nw_debug_trace. */
int rt_nw_debug_hits(rt_nw_ctx *ctx, const float *rays, const uint64_t *keys, int32_t n, int32_t *out_id, float *out_t,
                     int32_t *out_face);
/* Validation: the hit record of n given rays — the closest hit as
 * rt_nw_debug_hits resolves it, then the record a render makes of it.  Out per
 * ray: the winner's insertion index, t, out_pnuv = {p.xyz, n.xyz, u, v} (world
 * space; u, v are 0 unless the material's texture reads them) and the
 * material; a miss writes index -1 and zeros. */
int rt_nw_debug_records(rt_nw_ctx *ctx, const float *rays, const uint64_t *keys, int32_t n, int32_t *out_id, float *out_t,
                        float *out_pnuv /* 8 floats per ray */, int32_t *out_mat);
/* world.hit calls of the last render (waits for it). */
int rt_nw_ctx_last_segments(rt_nw_ctx *ctx, uint64_t *segments);
/* Diagnostic: the kernel of the last render, {persistent, uniform grid,
 * spheres-only instantiation (spheres and moving spheres, no instances or
 * media, solid / checker textures: the other kinds' code compiled out),
 * samples per work item}.  Same image for every choice. */
int rt_nw_ctx_last_kernel(rt_nw_ctx *ctx, int32_t *out4);
/* Diagnostic: the instantiation family the resident scene renders with — 0 no
 * triangle, 1 triangles, 2 triangles with attribute records, 3 placements of
 * shared meshes, 4 placements of which at least one moves, 5 placements of
 * which at least one is affine (rt_nw_transform). */
int rt_nw_ctx_scene_tri(rt_nw_ctx *ctx, int32_t *tri);
/* Diagnostic: what the last render's kernel walked from LDS, {BVH nodes,
 * object records} (1 / 0; the uniform grid stages the objects, no nodes). */
int rt_nw_ctx_last_staging(rt_nw_ctx *ctx, int32_t out2[2]);
/* Analysis builds only (-DRTMI_NW_PHASES=1): wave-level cycles of the loop
 * passes since the last call — closest hit, hit record + texture + scatter,
 * accumulation + regeneration, whole items; RT_EUNSUPPORTED otherwise. */
int rt_nw_debug_phases(uint64_t *out4);
/* Analysis: the executed work of the launches since the last call, counted
 * per lane by the RTMI_STATS build (librtmi_stats.so): {algorithmic FLOP of
 * the miss tests performed (per-kind counts as bench.py NW_FLOP) + 25 per
 * node slab test / grid clip + 5 per cell step, node visits, object tests,
 * cell steps}; zeroed after reading.  RT_EUNSUPPORTED in the product build. */
int rt_nw_debug_counters(uint64_t *out4);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_NW_H */
