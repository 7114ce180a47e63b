"""Next-Week renderer — Python view of include/rtmi_nw.h.

Mirrors the reference's rt_next_week/cuda/ vocabulary: a Scene is built with
one call per reference constructor and rendered by the gfx950 kernel; there
is no CPU fallback.

    s = Scene()
    white = s.lambertian(s.solid(.73, .73, .73))           # material.h:40-43
    box = s.translate(s.rotate_y(s.box((0, 0, 0), (165, 330, 165), white), 15), (265, 0, 295))
    s.add(s.constant_medium(box, 0.01, s.solid(0, 0, 0)))   # constant_medium.h
    cam = camera((278, 278, -800), (278, 278, 0), (0, 1, 0), 40, 1.0, 0.0, 800.0)
    sums = NwRenderer(s).render(cam, W, H, spp)

or a reference scene: `s, cam = preset(8, image=earth_rgb, aspect=1.0)`
(create_world main.cu:415-490).
"""
import ctypes as C

import numpy as np

from ._abi import (NW_ADAPT_ON_PASS, NW_DENOISE_DEMODULATE, NW_DENOISE_NO_EDGES, RtNwAdaptStats, RtNwCamera, RtNwDenoiseParams,
                   RtNwFlat, check, load)

__all__ = ["Scene", "NwRenderer", "camera", "preset", "obj_stage", "xorwow_uniforms", "load_image", "accum_info", "SCENES",
           "adapt_criterion", "adapt_info", "ADAPT_FLOOR", "adapt_variance", "denoise_params"]

_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
_u8 = C.POINTER(C.c_uint8)

# create_world's switch cases (main.cu:433-484)
SCENES = {"random": 1, "two_spheres": 2, "two_perlin_spheres": 3, "earth": 4, "simple_light": 5,
          "cornell_box": 6, "cornell_smoke": 7, "final": 8}


def _v3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def _id(rc, what):
    if rc < 0:
        check(rc, what)
    return rc


def camera(lookfrom, lookat, vup, vfov, aspect, aperture, focus_dist, time0=0.0, time1=1.0):
    """camera::camera camera.h:24-62 with the shutter [time0, time1]."""
    cam = RtNwCamera()
    check(load().rt_nw_camera_init(C.byref(cam), _v3(lookfrom), _v3(lookat), _v3(vup), float(vfov), float(aspect),
                                   float(aperture), float(focus_dist), float(time0), float(time1)), "rt_nw_camera_init")
    return cam


class Scene:
    """Host-side scene under construction (rt_nw_scene)."""

    def __init__(self):
        self._h = C.c_void_p()
        check(load().rt_nw_scene_create(C.byref(self._h)), "rt_nw_scene_create")

    # textures texture.h
    def solid(self, r, g, b):
        return _id(load().rt_nw_tex_solid(self._h, r, g, b), "rt_nw_tex_solid")

    def checker(self, even, odd):
        return _id(load().rt_nw_tex_checker(self._h, even, odd), "rt_nw_tex_checker")

    def noise(self, scale, ranvec, perm):
        rv = np.ascontiguousarray(ranvec, np.float32).reshape(256 * 3)
        pm = np.ascontiguousarray(perm, np.int32).reshape(3 * 256)
        return _id(load().rt_nw_tex_noise(self._h, float(scale), rv.ctypes.data_as(_fp), pm.ctypes.data_as(_ip)),
                   "rt_nw_tex_noise")

    def image(self, rgb):
        if rgb is None:
            return _id(load().rt_nw_tex_image(self._h, None, 0, 0), "rt_nw_tex_image")
        a = np.ascontiguousarray(rgb, np.uint8)
        h, w = a.shape[:2]
        return _id(load().rt_nw_tex_image(self._h, a.ctypes.data_as(_u8), w, h), "rt_nw_tex_image")

    # materials material.h
    def lambertian(self, tex):
        return _id(load().rt_nw_mat_lambertian(self._h, tex), "rt_nw_mat_lambertian")

    def metal(self, tex, fuzz):
        return _id(load().rt_nw_mat_metal(self._h, tex, float(fuzz)), "rt_nw_mat_metal")

    def dielectric(self, ir):
        return _id(load().rt_nw_mat_dielectric(self._h, float(ir)), "rt_nw_mat_dielectric")

    def diffuse_light(self, tex):
        return _id(load().rt_nw_mat_diffuse_light(self._h, tex), "rt_nw_mat_diffuse_light")

    def isotropic(self, tex):
        return _id(load().rt_nw_mat_isotropic(self._h, tex), "rt_nw_mat_isotropic")

    # objects
    def sphere(self, center, radius, mat):
        return _id(load().rt_nw_sphere(self._h, _v3(center), float(radius), mat), "rt_nw_sphere")

    def moving_sphere(self, c0, c1, t0, t1, radius, mat):
        return _id(load().rt_nw_moving_sphere(self._h, _v3(c0), _v3(c1), float(t0), float(t1), float(radius), mat),
                   "rt_nw_moving_sphere")

    def rect(self, plane, a0, a1, b0, b1, k, mat):
        """plane 'xy' | 'xz' | 'yz' (aarect.h)."""
        p = {"xy": 0, "xz": 1, "yz": 2}[plane]
        return _id(load().rt_nw_rect(self._h, p, a0, a1, b0, b1, k, mat), "rt_nw_rect")

    def box(self, p0, p1, mat):
        return _id(load().rt_nw_box(self._h, _v3(p0), _v3(p1), mat), "rt_nw_box")

    def triangle(self, v0, v1, v2, mat):
        """A two-sided, watertight triangle; counter-clockwise is front."""
        return _id(load().rt_nw_triangle(self._h, _v3(v0), _v3(v1), _v3(v2), mat), "rt_nw_triangle")

    def mesh(self, verts, faces, normals=None, mat=None, normal_faces=None, uvs=None, uv_faces=None, smooth=False,
             gen_normals=False):
        """Triangles `faces` (n x 3 vertex indices) over `verts` (m x 3) as
        one handle; `normals` (k x 3), indexed by `normal_faces` (n x 3) or,
        without it, by the vertex indices, fix the winding (rt_nw_mesh).
        smooth: shade with the interpolated normals (gen_normals: area-weighted
        vertex normals where none is given); uvs (k x 2), indexed by uv_faces
        or the vertex indices: texture coordinates (rt_nw_mesh_attr)."""
        if mat is None:
            raise TypeError("Scene.mesh: mat is required")
        v = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
        f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
        nf = None if normal_faces is None else np.ascontiguousarray(normal_faces, np.int32).reshape(-1, 3)
        if nf is not None and len(nf) != len(f):
            raise ValueError("Scene.mesh: normal_faces must have one row per face")
        if uvs is None and uv_faces is None and not smooth and not gen_normals:
            return _id(load().rt_nw_mesh(self._h, v.ctypes.data_as(_dp), len(v), f.ctypes.data_as(_ip), len(f),
                                         None if nrm is None else nrm.ctypes.data_as(_dp), 0 if nrm is None else len(nrm),
                                         None if nf is None else nf.ctypes.data_as(_ip), mat), "rt_nw_mesh")
        uv = None if uvs is None else np.ascontiguousarray(uvs, np.float64).reshape(-1, 2)
        uf = None if uv_faces is None else np.ascontiguousarray(uv_faces, np.int32).reshape(-1, 3)
        if uf is not None and len(uf) != len(f):
            raise ValueError("Scene.mesh: uv_faces must have one row per face")
        return self.mesh_attr(v, f, nrm, nf, uv, uf, _mesh_flags(smooth, uv is not None, gen_normals), mat)

    def mesh_attr(self, v, f, nrm, nf, uv, uf, flags, mat):
        """rt_nw_mesh_attr as it is (contiguous arrays or None, RT_NW_MESH_* flags)."""
        return _id(load().rt_nw_mesh_attr(self._h, v.ctypes.data_as(_dp), len(v), f.ctypes.data_as(_ip), len(f),
                                          None if nrm is None else nrm.ctypes.data_as(_dp), 0 if nrm is None else len(nrm),
                                          None if nf is None else nf.ctypes.data_as(_ip),
                                          None if uv is None else uv.ctypes.data_as(_dp), 0 if uv is None else len(uv),
                                          None if uf is None else uf.ctypes.data_as(_ip), flags, mat), "rt_nw_mesh_attr")

    def load_obj(self, path, mat, smooth=False, uv=False, gen_normals=False):
        """A Wavefront OBJ file as one mesh: (handle, triangle count).  smooth /
        gen_normals: shade with the file's vn (generated where missing); uv:
        read vt and the corners' t (rt_nw_load_obj_attr); none of them:
        rt_nw_load_obj."""
        n = C.c_int32()
        if not (smooth or uv or gen_normals):
            h = _id(load().rt_nw_load_obj(self._h, str(path).encode(), mat, C.byref(n)), "rt_nw_load_obj")
        else:
            h = _id(load().rt_nw_load_obj_attr(self._h, str(path).encode(), mat, _mesh_flags(smooth, uv, gen_normals),
                                               C.byref(n)), "rt_nw_load_obj_attr")
        return h, n.value

    def flat_attr(self):
        """The triangle attribute records beside flat() (rt_nw_scene_flat_attr):
        {"attr": float32 n x 16 (normals 9, uvs 6, flags as int bits),
        "attr_of_obj": int32 per flattened object, -1: none}."""
        n, a, o = C.c_int32(), _fp(), _ip()
        fl = RtNwFlat()  # (the object count; taken first: a flat view at another time invalidates the pointers)
        check(load().rt_nw_scene_flat(self._h, C.byref(fl)), "rt_nw_scene_flat")
        check(load().rt_nw_scene_flat_attr(self._h, C.byref(n), C.byref(a), C.byref(o)), "rt_nw_scene_flat_attr")
        attr = np.ctypeslib.as_array(a, shape=(16 * n.value,)).copy() if n.value else np.zeros(0, np.float32)
        of = np.ctypeslib.as_array(o, shape=(fl.n_obj,)).copy() if fl.n_obj else np.zeros(0, np.int32)
        return {"attr": attr.astype(np.float32).reshape(-1, 16), "attr_of_obj": of.astype(np.int32)}

    def constant_medium(self, boundary, density, tex):
        return _id(load().rt_nw_constant_medium(self._h, boundary, float(density), tex), "rt_nw_constant_medium")

    def group(self, objs):
        a = np.ascontiguousarray(objs, np.int32)
        return _id(load().rt_nw_group(self._h, a.ctypes.data_as(_ip), a.size), "rt_nw_group")

    def translate(self, obj, offset):
        return _id(load().rt_nw_translate(self._h, obj, _v3(offset)), "rt_nw_translate")

    def rotate_y(self, obj, angle):
        return _id(load().rt_nw_rotate_y(self._h, obj, float(angle)), "rt_nw_rotate_y")

    def shared(self, obj):
        """`obj` (triangles, meshes and groups of them) as shared geometry: a
        handle to translate, rotate_y, group and add any number of times; the
        device holds the triangles once and one small record per placement, and
        the image is that of the copies, bit for bit (rt_nw_shared)."""
        return _id(load().rt_nw_shared(self._h, obj), "rt_nw_shared")

    def move(self, obj, off0, off1, t0=0.0, t1=1.0):
        """A translate node whose offset is linear in the ray's time: off0 at t0,
        off1 at t1 (rt_nw_move).  `obj`: one shared handle, optionally under
        translate / rotate_y nodes."""
        return _id(load().rt_nw_move(self._h, obj, _v3(off0), _v3(off1), float(t0), float(t1)), "rt_nw_move")

    def transform(self, obj, m):
        """A placement node with the affine map world = A local + b (rt_nw_transform).
        m: 3 x 4 (A | b), or 4 x 4 with the last row 0 0 0 1.  `obj`: one shared
        handle under translate / rotate_y / transform nodes and at most one move."""
        a = np.asarray(m, np.float64)
        if a.shape == (4, 4):
            if not np.array_equal(a[3], [0.0, 0.0, 0.0, 1.0]):
                raise ValueError("Scene.transform: the last row of a 4 x 4 matrix must be 0 0 0 1")
            a = a[:3]
        if a.shape != (3, 4):
            raise ValueError("Scene.transform: a 3 x 4 or 4 x 4 matrix")
        a = np.ascontiguousarray(a)
        return _id(load().rt_nw_transform(self._h, obj, a.ctypes.data_as(C.POINTER(C.c_double))), "rt_nw_transform")

    def affine_stats(self):
        """(affine placements reached from the world, other placements) (rt_nw_scene_affine_stats)."""
        v = (C.c_int32 * 2)()
        check(load().rt_nw_scene_affine_stats(self._h, v), "rt_nw_scene_affine_stats")
        return v[0], v[1]

    def motion_stats(self):
        """(moving placements reached from the world, static placements) (rt_nw_scene_motion_stats)."""
        v = (C.c_int32 * 2)()
        check(load().rt_nw_scene_motion_stats(self._h, v), "rt_nw_scene_motion_stats")
        return v[0], v[1]

    def add(self, obj):
        check(load().rt_nw_world_add(self._h, obj), "rt_nw_world_add")
        return self

    def set_background(self, r, g, b):
        check(load().rt_nw_set_background(self._h, r, g, b), "rt_nw_set_background")

    def flat(self, time=None):
        """The flattened scene (what the GPU renders), as numpy arrays (copies).
        time: the instant moving placements (Scene.move) are expanded at
        (rt_nw_scene_flat_at); None: rt_nw_scene_flat, which is time 0."""
        f = RtNwFlat()
        if time is None:
            check(load().rt_nw_scene_flat(self._h, C.byref(f)), "rt_nw_scene_flat")
        else:
            check(load().rt_nw_scene_flat_at(self._h, float(time), C.byref(f)), "rt_nw_scene_flat_at")

        def arr(p, n, dt=np.float32):
            return np.ctypeslib.as_array(p, shape=(n,)).astype(dt).copy() if n else np.zeros(0, dt)

        return {
            "obj": arr(f.obj, 16 * f.n_obj), "inst": arr(f.inst, 8 * f.n_inst), "mat": arr(f.mat, 4 * f.n_mat),
            "tex": arr(f.tex, 8 * f.n_tex), "perlin_vec": arr(f.perlin_vec, 1024 * f.n_perlin),
            "perlin_perm": arr(f.perlin_perm, 768 * f.n_perlin, np.int32),
            "image_desc": arr(f.image_desc, 4 * f.n_image, np.int32),
            "image_px": arr(f.image_px, int(f.image_bytes), np.uint8),
            "background": np.array(list(f.background), np.float32),
            "n_obj": f.n_obj,
        }

    def hash(self):
        """FNV-1a 64 over everything of the scene that can change a pixel (host
        only, rt_nw_scene_hash): what a checkpoint is tied to.  Equal in any two
        processes that build the scene with the same calls."""
        v = C.c_uint64()
        check(load().rt_nw_scene_hash(self._h, C.byref(v)), "rt_nw_scene_hash")
        return v.value

    def grid_stats(self):
        """The uniform grid a device context would build (host only,
        rt_nw_scene_grid_stats): {"dims", "max_cell", "n_big", "n_refs"}."""
        dims = (C.c_int32 * 3)()
        mc, nb, nr = C.c_int32(), C.c_int32(), C.c_int32()
        check(load().rt_nw_scene_grid_stats(self._h, dims, C.byref(mc), C.byref(nb), C.byref(nr)),
              "rt_nw_scene_grid_stats")
        return {"dims": tuple(dims), "max_cell": mc.value, "n_big": nb.value, "n_refs": nr.value}

    def instancing_stats(self):
        """What a device context would build of the shared meshes (host only,
        rt_nw_scene_instancing_stats): {"meshes", "placements", "pool_triangles",
        "bottom_nodes", "top_leaves", "top_nodes"}; the first four are 0 in a
        scene without a placement."""
        v = (C.c_int32 * 6)()
        check(load().rt_nw_scene_instancing_stats(self._h, v), "rt_nw_scene_instancing_stats")
        return dict(zip(("meshes", "placements", "pool_triangles", "bottom_nodes", "top_leaves", "top_nodes"), list(v)))

    def close(self):
        if self._h:
            load().rt_nw_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def preset(which, image=None, aspect=1.0, rtl=False):
    """The reference's scene `which` (name or create_world case 1..8) and its camera."""
    w = SCENES.get(which, which)
    s = Scene()
    cam = RtNwCamera()
    if image is not None:
        a = np.ascontiguousarray(image, np.uint8)
        s._img = a
        ptr, ih, iw = a.ctypes.data_as(_u8), a.shape[0], a.shape[1]
    else:
        ptr, ih, iw = None, 0, 0
    check(load().rt_nw_scene_preset(s._h, int(w), ptr, iw, ih, float(aspect), 1 if rtl else 0, C.byref(cam)),
          "rt_nw_scene_preset")
    return s, cam


def _mesh_flags(smooth, uv, gen_normals):
    """RT_NW_MESH_SMOOTH | _UV | _GEN_NORMALS."""
    return (1 if smooth else 0) | (2 if uv else 0) | (4 if gen_normals else 0)


def affine(scale=1.0, axis=(0, 1, 0), angle=0.0, translate=(0, 0, 0)):
    """The 3 x 4 matrix of Scene.transform for: scale (a scalar or three values,
    along x, y, z), then a rotation of `angle` degrees about `axis`, then the
    translation."""
    sc = np.broadcast_to(np.asarray(scale, np.float64), (3,))
    ax = np.asarray(axis, np.float64)
    ax = ax / np.linalg.norm(ax)
    th = np.deg2rad(float(angle))
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    return np.concatenate([R @ np.diag(sc), np.asarray(translate, np.float64).reshape(3, 1)], axis=1)


def obj_stage(path, mat="lambertian", aspect=1.0, smooth=False, gen_normals=False, texture=None, copies=1, move=None,
              tumble=False):
    """The scene of `rtmi_nw_render --obj FILE --obj-mat MAT` and its camera:
    (scene, camera, triangle count).  smooth / gen_normals as Scene.load_obj;
    texture (h x w x 3 uint8): the mesh's texture, mapped by the file's vt
    (rt_nw_scene_obj_stage_attr; none of them: rt_nw_scene_obj_stage).
    copies = N > 1 (`--obj-copies N`): the model as one shared mesh placed in an
    N x N field (rt_nw_scene_obj_stage_copies).  move (`--obj-move DX,DY,DZ`):
    every placement moves by that vector over [0, 1]
    (rt_nw_scene_obj_stage_moving)."""
    kind = {"lambertian": 0, "metal": 1, "glass": 2, "dielectric": 2}[mat]
    s = Scene()
    cam = RtNwCamera()
    n = C.c_int32()
    if tumble:  # (`--obj-tumble`: every copy an affine placement, rt_nw_scene_obj_stage_tumbled)
        if texture is not None:
            a = np.ascontiguousarray(texture, np.uint8)
            ptr, ih, iw = a.ctypes.data_as(_u8), a.shape[0], a.shape[1]
        else:
            ptr, ih, iw = None, 0, 0
        check(load().rt_nw_scene_obj_stage_tumbled(s._h, str(path).encode(), kind,
                                                   _mesh_flags(smooth, texture is not None, gen_normals), ptr, iw, ih,
                                                   int(copies), None if move is None else _v3(move), float(aspect),
                                                   C.byref(cam), C.byref(n)),
              "rt_nw_scene_obj_stage_tumbled")
        return s, cam, n.value
    if move is not None:
        if texture is not None:
            a = np.ascontiguousarray(texture, np.uint8)
            ptr, ih, iw = a.ctypes.data_as(_u8), a.shape[0], a.shape[1]
        else:
            ptr, ih, iw = None, 0, 0
        check(load().rt_nw_scene_obj_stage_moving(s._h, str(path).encode(), kind,
                                                  _mesh_flags(smooth, texture is not None, gen_normals), ptr, iw, ih,
                                                  int(copies), _v3(move), float(aspect), C.byref(cam), C.byref(n)),
              "rt_nw_scene_obj_stage_moving")
        return s, cam, n.value
    if copies != 1:
        if texture is not None:
            a = np.ascontiguousarray(texture, np.uint8)
            ptr, ih, iw = a.ctypes.data_as(_u8), a.shape[0], a.shape[1]
        else:
            ptr, ih, iw = None, 0, 0
        check(load().rt_nw_scene_obj_stage_copies(s._h, str(path).encode(), kind,
                                                  _mesh_flags(smooth, texture is not None, gen_normals), ptr, iw, ih,
                                                  int(copies), float(aspect), C.byref(cam), C.byref(n)),
              "rt_nw_scene_obj_stage_copies")
        return s, cam, n.value
    if not (smooth or gen_normals) and texture is None:
        check(load().rt_nw_scene_obj_stage(s._h, str(path).encode(), kind, float(aspect), C.byref(cam), C.byref(n)),
              "rt_nw_scene_obj_stage")
        return s, cam, n.value
    if texture is not None:
        a = np.ascontiguousarray(texture, np.uint8)
        ptr, ih, iw = a.ctypes.data_as(_u8), a.shape[0], a.shape[1]
    else:
        ptr, ih, iw = None, 0, 0
    check(load().rt_nw_scene_obj_stage_attr(s._h, str(path).encode(), kind, _mesh_flags(smooth, texture is not None, gen_normals),
                                            ptr, iw, ih, float(aspect), C.byref(cam), C.byref(n)),
          "rt_nw_scene_obj_stage_attr")
    return s, cam, n.value


def xorwow_uniforms(n, seed=1984):
    """curand_init(seed, 0, 0) + n x curand_uniform, restated (the scene generator's stream)."""
    out = np.zeros(n, np.float32)
    check(load().rt_nw_xorwow_uniforms(seed, n, out.ctypes.data_as(_fp)), "rt_nw_xorwow_uniforms")
    return out


def accum_info(path):
    """The header of a Next-Week checkpoint file (host only, rt_nw_accum_info)."""
    v, u = (C.c_int32 * 8)(), (C.c_uint64 * 3)()
    check(load().rt_nw_accum_info(str(path).encode(), v, u), "rt_nw_accum_info")
    d = dict(zip(("W", "H", "row0", "row_step", "nrows", "spp_done", "max_depth", "zero"), list(v)))
    d.update(zip(("seed", "scene_hash", "camera_hash"), list(u)))
    return d


def adapt_info(path):
    """The header of a Next-Week adaptive checkpoint file (host only, rt_nw_adapt_info);
    spp_done is the largest count a pixel holds."""
    v, u = (C.c_int32 * 8)(), (C.c_uint64 * 3)()
    check(load().rt_nw_adapt_info(str(path).encode(), v, u), "rt_nw_adapt_info")
    d = dict(zip(("W", "H", "row0", "row_step", "nrows", "spp_done", "max_depth", "zero"), list(v)))
    d.update(zip(("seed", "scene_hash", "camera_hash"), list(u)))
    return d


# The channel-sum level below which adapt_criterion judges the error absolutely: a mean of 0.01 per channel,
# level 25 of 255 after the square-root transfer (rtmi_nw.h).
ADAPT_FLOOR = 0.03


def adapt_criterion(s, m2, n, min_spp, max_spp, threshold, floor=ADAPT_FLOOR, dilate=1):
    """Which pixels need more samples (host only, rt_nw_adapt_criterion): from
    sum [nrows, W, 3], m2 and n [nrows, W] to (active uint8 [nrows, W], err
    float64 [nrows, W], active count)."""
    n = np.ascontiguousarray(n, np.int32)
    if n.ndim != 2:
        raise ValueError("adapt_criterion: n must be [nrows, W]")
    s, m2 = np.ascontiguousarray(s, np.int64), np.ascontiguousarray(m2, np.uint64)
    if s.shape != n.shape + (3,) or m2.shape != n.shape:
        raise ValueError("adapt_criterion: sum [nrows, W, 3], m2 and n [nrows, W]")
    active, err, count = np.zeros(n.shape, np.uint8), np.zeros(n.shape, np.float64), C.c_int64()
    check(load().rt_nw_adapt_criterion(s.ctypes.data_as(C.POINTER(C.c_int64)), m2.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       n.ctypes.data_as(_ip), n.shape[1], n.shape[0], min_spp, max_spp, float(threshold),
                                       float(floor), dilate, active.ctypes.data_as(_u8), err.ctypes.data_as(_dp),
                                       C.byref(count)), "rt_nw_adapt_criterion")
    return active, err, count.value


def adapt_variance(s, m2, n):
    """The variance of each pixel's mean channel sum (host only, rt_nw_adapt_variance),
    the denoiser's guide: from sum [nrows, W, 3], m2 and n [nrows, W] to float32
    [nrows, W]; +inf where n < 2."""
    n = np.ascontiguousarray(n, np.int32)
    if n.ndim != 2:
        raise ValueError("adapt_variance: n must be [nrows, W]")
    s, m2 = np.ascontiguousarray(s, np.int64), np.ascontiguousarray(m2, np.uint64)
    if s.shape != n.shape + (3,) or m2.shape != n.shape:
        raise ValueError("adapt_variance: sum [nrows, W, 3], m2 and n [nrows, W]")
    var = np.zeros(n.shape, np.float32)
    check(load().rt_nw_adapt_variance(s.ctypes.data_as(C.POINTER(C.c_int64)), m2.ctypes.data_as(C.POINTER(C.c_uint64)),
                                      n.ctypes.data_as(_ip), n.shape[1], n.shape[0], var.ctypes.data_as(_fp)),
          "rt_nw_adapt_variance")
    return var


def denoise_params(iterations=None, sigma_l=None, sigma_n=None, sigma_z=None, demodulate=None, no_edges=False, validate=True):
    """rt_nw_denoise_params: the library's defaults (5 iterations, sigma_l 4,
    sigma_n 128, sigma_z 1, demodulation on) with the given fields replaced,
    checked by rt_nw_denoise_params_check (host only)."""
    p = RtNwDenoiseParams()
    check(load().rt_nw_denoise_params_default(C.byref(p)), "rt_nw_denoise_params_default")
    for name, v in (("iterations", iterations), ("sigma_l", sigma_l), ("sigma_n", sigma_n), ("sigma_z", sigma_z)):
        if v is not None:
            setattr(p, name, v)
    if demodulate is not None:
        p.flags = (p.flags & ~NW_DENOISE_DEMODULATE) | (NW_DENOISE_DEMODULATE if demodulate else 0)
    if no_edges:
        p.flags |= NW_DENOISE_NO_EDGES
    if validate:
        check(load().rt_nw_denoise_params_check(C.byref(p)), "rt_nw_denoise_params_check")
    return p


def load_image(path):
    """Decode an image file (the earth texture) to h x w x 3 uint8, row 0 at the top (PIL)."""
    from PIL import Image

    return np.asarray(Image.open(path).convert("RGB"), np.uint8)


class NwRenderer:
    """One device context with a resident Next-Week scene (rt_nw_ctx)."""

    def __init__(self, scene, device=0):
        self._h = C.c_void_p()
        check(load().rt_nw_ctx_create(device, C.byref(self._h)), "rt_nw_ctx_create")
        self.set_scene(scene)

    def set_scene(self, scene):
        check(load().rt_nw_ctx_set_scene(self._h, scene._h), "rt_nw_ctx_set_scene")
        self._scene = scene  # (checkpoints carry its hash)

    def info(self):
        a, b = C.c_int32(), C.c_int32()
        check(load().rt_nw_ctx_info(self._h, C.byref(a), C.byref(b)), "rt_nw_ctx_info")
        return a.value, b.value

    ACCELS = {"auto": 0, "bvh": 1, "grid": 2}

    def set_accel(self, kind):
        """Closest-hit structure: "auto" (the grid when balanced, else the BVH),
        "bvh" or "grid" (rt_nw_ctx_set_accel); the same image either way."""
        check(load().rt_nw_ctx_set_accel(self._h, self.ACCELS[kind]), "rt_nw_ctx_set_accel")

    def accel_info(self):
        """{"accel": the structure renders use, "dims": grid cells per axis
        (zeros: no grid), "max_cell": fullest cell, "n_big": brute-force list}."""
        used, mc, nb = C.c_int32(), C.c_int32(), C.c_int32()
        dims = (C.c_int32 * 3)()
        check(load().rt_nw_ctx_accel_info(self._h, C.byref(used), dims, C.byref(mc), C.byref(nb)),
              "rt_nw_ctx_accel_info")
        names = {v: k for k, v in self.ACCELS.items()}
        return {"accel": names[used.value], "dims": tuple(dims), "max_cell": mc.value, "n_big": nb.value}

    def render(self, cam, W, H, spp, max_depth=50, seed=1984):
        out = np.zeros((H, W, 3), np.float32)
        check(load().rt_nw_render(self._h, C.byref(cam), W, H, spp, max_depth, seed, out.ctypes.data_as(_fp)),
              "rt_nw_render")
        return out

    def render_rows(self, cam, W, H, spp, max_depth, seed, row0, row_step, nrows, dev_ptr, stream=0):
        check(load().rt_nw_render_rows(self._h, C.byref(cam), W, H, spp, max_depth, seed, row0, row_step, nrows,
                                       C.c_void_p(dev_ptr), C.c_void_p(stream)), "rt_nw_render_rows")

    # ---- progressive passes (rt_nw_accum_* / rt_nw_render_pass) -----------
    def accum_reset(self, W, nrows):
        """A zeroed accumulator for a W x nrows strip (whole image: nrows = H)."""
        check(load().rt_nw_accum_reset(self._h, W, nrows), "rt_nw_accum_reset")
        self._acc_shape = (nrows, W, 3)

    def render_pass(self, cam, W, H, s_begin, s_count, max_depth=50, seed=1984, row0=0, row_step=1, nrows=None, stream=0):
        """Add samples [s_begin, s_begin + s_count) of the rows to the accumulator (async)."""
        nrows = H if nrows is None else nrows
        check(load().rt_nw_render_pass(self._h, C.byref(cam), W, H, s_begin, s_count, max_depth, seed, row0, row_step,
                                       nrows, C.c_void_p(stream)), "rt_nw_render_pass")

    def resolve(self, dev_ptr=None, stream=0):
        """The accumulator as float sums: into the device strip dev_ptr
        (asynchronous on `stream`), else returned as a host array [nrows, W, 3].
        The accumulator is unchanged, so more passes may follow."""
        if dev_ptr is not None:
            check(load().rt_nw_accum_resolve(self._h, C.c_void_p(dev_ptr), None, C.c_void_p(stream)), "rt_nw_accum_resolve")
            return None
        out = np.zeros(getattr(self, "_acc_shape", (0, 0, 3)), np.float32)
        check(load().rt_nw_accum_resolve(self._h, None, out.ctypes.data_as(_fp), C.c_void_p(stream)), "rt_nw_accum_resolve")
        return out

    def accum_export(self):
        """(raw int64 fixed-point sums [nrows, W, 3], samples accumulated)."""
        raw = np.zeros(getattr(self, "_acc_shape", (0, 0, 3)), np.int64)
        done = C.c_int32()
        check(load().rt_nw_accum_export(self._h, raw.ctypes.data_as(C.POINTER(C.c_int64)), raw.size, C.byref(done)),
              "rt_nw_accum_export")
        return raw, done.value

    def accum_import(self, raw, spp_done):
        raw = np.ascontiguousarray(raw, np.int64)
        check(load().rt_nw_accum_import(self._h, raw.ctypes.data_as(C.POINTER(C.c_int64)), raw.size, spp_done),
              "rt_nw_accum_import")

    def progressive(self, cam, W, H, spp, pass_spp, max_depth=50, seed=1984, checkpoint=None, on_pass=None,
                    row0=0, row_step=1, nrows=None):
        """Samples [0, spp) in passes of pass_spp (each a bounded kernel), resuming
        from `checkpoint` when that file exists and saving to it after every pass;
        on_pass(done) is called after each.  Returns the float sums [nrows, W, 3]:
        bit-identical to render(spp) for any pass split (as Renderer.progressive)."""
        import os

        if pass_spp < 1:
            raise ValueError("pass_spp must be at least 1")
        nrows = H if nrows is None else nrows
        self.accum_reset(W, nrows)
        L, sc = load(), self._scene._h
        done = 0
        if checkpoint and os.path.exists(checkpoint):
            n = C.c_int32()
            check(L.rt_nw_accum_load(self._h, str(checkpoint).encode(), sc, C.byref(cam), W, H, row0, row_step, nrows,
                                     max_depth, seed, C.byref(n)), "rt_nw_accum_load")
            done = n.value
        while done < spp:
            k = min(pass_spp, spp - done)
            self.render_pass(cam, W, H, done, k, max_depth, seed, row0, row_step, nrows)
            done += k
            if checkpoint:  # (waits for the pass)
                check(L.rt_nw_accum_save(self._h, str(checkpoint).encode(), sc, C.byref(cam), H, row0, row_step, max_depth,
                                         seed), "rt_nw_accum_save")
            if on_pass is not None:
                on_pass(done)
        return self.resolve()

    # ---- adaptive sampling (rt_nw_adapt_*) --------------------------------
    def adapt_reset(self, W, nrows):
        """A zeroed adaptive accumulator (colour sums, second moments, counts) for a W x nrows strip."""
        check(load().rt_nw_adapt_reset(self._h, W, nrows), "rt_nw_adapt_reset")
        self._adapt_shape = (nrows, W)

    def adapt_pass(self, cam, W, H, s_count, max_depth=50, seed=1984, row0=0, row_step=1, nrows=None, active=None, stream=0):
        """Give every active pixel p the samples [n[p], n[p] + s_count) (async).
        active: [nrows, W], nonzero = sample this pixel; None = all."""
        nrows = H if nrows is None else nrows
        ptr = None
        if active is not None:
            m = np.ascontiguousarray(np.asarray(active) != 0, np.uint8)
            if m.shape != (nrows, W):
                raise ValueError("adapt_pass: active must be [nrows, W]")
            ptr = m.ctypes.data_as(_u8)
        check(load().rt_nw_adapt_pass(self._h, C.byref(cam), W, H, s_count, max_depth, seed, row0, row_step, nrows, ptr,
                                      C.c_void_p(stream)), "rt_nw_adapt_pass")

    def adapt_export(self):
        """(sum int64 [nrows, W, 3], m2 uint64 [nrows, W], n int32 [nrows, W])."""
        sh = getattr(self, "_adapt_shape", (0, 0))
        s, m2, n = np.zeros(sh + (3,), np.int64), np.zeros(sh, np.uint64), np.zeros(sh, np.int32)
        check(load().rt_nw_adapt_export(self._h, s.ctypes.data_as(C.POINTER(C.c_int64)), m2.ctypes.data_as(C.POINTER(C.c_uint64)),
                                        n.ctypes.data_as(_ip), n.size), "rt_nw_adapt_export")
        return s, m2, n

    def adapt_import(self, s, m2, n):
        s, m2, n = np.ascontiguousarray(s, np.int64), np.ascontiguousarray(m2, np.uint64), np.ascontiguousarray(n, np.int32)
        if s.size != 3 * n.size or m2.size != n.size:
            raise ValueError("adapt_import: sum [nrows, W, 3], m2 and n [nrows, W]")
        check(load().rt_nw_adapt_import(self._h, s.ctypes.data_as(C.POINTER(C.c_int64)), m2.ctypes.data_as(C.POINTER(C.c_uint64)),
                                        n.ctypes.data_as(_ip), n.size), "rt_nw_adapt_import")

    def adapt_resolve(self, dev_ptr=None, stream=0):
        """The per-pixel means float(double(sum) * 2^-32 / n), 0 where n = 0: into
        the device strip dev_ptr (asynchronous), else a host array [nrows, W, 3]."""
        if dev_ptr is not None:
            check(load().rt_nw_adapt_resolve(self._h, C.c_void_p(dev_ptr), None, C.c_void_p(stream)), "rt_nw_adapt_resolve")
            return None
        out = np.zeros(getattr(self, "_adapt_shape", (0, 0)) + (3,), np.float32)
        check(load().rt_nw_adapt_resolve(self._h, None, out.ctypes.data_as(_fp), C.c_void_p(stream)), "rt_nw_adapt_resolve")
        return out

    def adapt_save(self, path, cam, H, max_depth=50, seed=1984, row0=0, row_step=1):
        check(load().rt_nw_adapt_save(self._h, str(path).encode(), self._scene._h, C.byref(cam), H, row0, row_step, max_depth,
                                      seed), "rt_nw_adapt_save")

    def adapt_load(self, path, cam, W, H, max_depth=50, seed=1984, row0=0, row_step=1, nrows=None):
        nrows = H if nrows is None else nrows
        check(load().rt_nw_adapt_load(self._h, str(path).encode(), self._scene._h, C.byref(cam), W, H, row0, row_step, nrows,
                                      max_depth, seed), "rt_nw_adapt_load")
        self._adapt_shape = (nrows, W)

    # ---- denoising (rt_nw_render_features / rt_nw_denoise) ----------------
    def features(self, cam, W, H, fspp=16, seed=1984):
        """First-hit feature buffers [H, W, 8] float32, row 0 at the bottom: mean
        albedo rgb, mean normal xyz (not unit), mean t of the hits and coverage
        over fspp camera samples per pixel (rt_nw_render_features)."""
        out = np.zeros((H, W, 8), np.float32)
        check(load().rt_nw_render_features(self._h, C.byref(cam), W, H, fspp, seed, None, out.ctypes.data_as(_fp), None),
              "rt_nw_render_features")
        return out

    def denoise(self, mean, var, feat, var_out=False, **params):
        """The edge-avoiding a-trous filter (rt_nw_denoise_host) of mean [H, W, 3]
        guided by feat [H, W, 8] and var [H, W] (the variance of the mean channel
        sum, adapt_variance; None: no luminance term).  params: denoise_params'
        keywords.  Returns the filtered image, and with var_out=True (needs var)
        also the filtered variance."""
        mean = np.ascontiguousarray(mean, np.float32)
        feat = np.ascontiguousarray(feat, np.float32)
        if mean.ndim != 3 or mean.shape[2] != 3 or feat.shape != mean.shape[:2] + (8,):
            raise ValueError("denoise: mean [H, W, 3] and feat [H, W, 8]")
        H, W = mean.shape[:2]
        v = None
        if var is not None:
            v = np.ascontiguousarray(var, np.float32)
            if v.shape != (H, W):
                raise ValueError("denoise: var must be [H, W]")
        if var_out and v is None:
            raise ValueError("denoise: var_out needs var")
        p = denoise_params(validate=False, **params)
        out = np.zeros((H, W, 3), np.float32)
        vo = np.zeros((H, W), np.float32) if var_out else None
        check(load().rt_nw_denoise_host(self._h, W, H, mean.ctypes.data_as(_fp), None if v is None else v.ctypes.data_as(_fp),
                                        feat.ctypes.data_as(_fp), C.byref(p), out.ctypes.data_as(_fp),
                                        None if vo is None else vo.ctypes.data_as(_fp)), "rt_nw_denoise_host")
        return (out, vo) if var_out else out

    def adaptive(self, cam, W, H, min_spp, max_spp, pass_spp, threshold, floor=ADAPT_FLOOR, dilate=1, max_depth=50, seed=1984,
                 checkpoint=None, time_limit=None, on_pass=None, stats=None, denoise=False, fspp=16, denoise_args=None):
        """Sample until no pixel's relative error (adapt_criterion) exceeds
        `threshold`, no pixel above max_spp samples, in passes of pass_spp over
        the active pixels (rt_nw_render_adaptive); resumes from `checkpoint` when
        that file exists and saves to it after every pass; on_pass(pass number,
        pixels it sampled) is called after each, and an exception it raises ends
        the run and is raised again here; time_limit (seconds): no new pass after
        that long (one always runs).  Returns (mean [H, W, 3] float32, n [H, W]
        int32, err [H, W] float64); stats (a dict, when given) receives passes,
        stopped, total_samples, pixels_at_max, samples and segments (this call's)
        and active (pixels per pass).  denoise=True (rt_nw_render_denoised): a
        fourth value, the image filtered with features of fspp samples per pixel
        and denoise_args (denoise_params' keywords); the first three are unchanged."""
        mean, n, err = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.int32), np.zeros((H, W), np.float64)
        # (pixels join at different passes, so there can be more than max_spp / pass_spp of them; the log keeps
        # the first 4 max_spp / pass_spp + 64)
        log = np.zeros(4 * -(-max(max_spp, 1) // max(pass_spp, 1)) + 64, np.int64)
        st = RtNwAdaptStats(active=log.ctypes.data_as(C.POINTER(C.c_int64)), cap=log.size)
        raised = []

        def step(_user, k, count):
            try:
                on_pass(k, count)
            except BaseException as e:  # (must not cross the C frames)
                raised.append(e)
                return 1
            return 0

        cb = NW_ADAPT_ON_PASS(step) if on_pass is not None else NW_ADAPT_ON_PASS()
        args = (self._h, self._scene._h, C.byref(cam), W, H, min_spp, max_spp, pass_spp, float(threshold), float(floor), dilate,
                max_depth, seed, None if checkpoint is None else str(checkpoint).encode(),
                -1.0 if time_limit is None else float(time_limit), mean.ctypes.data_as(_fp), n.ctypes.data_as(_ip),
                err.ctypes.data_as(_dp), C.byref(st), cb, None)
        filtered = None
        if denoise:
            filtered = np.zeros((H, W, 3), np.float32)
            dp = denoise_params(validate=False, **(denoise_args or {}))
            check(load().rt_nw_render_denoised(*args, fspp, C.byref(dp), filtered.ctypes.data_as(_fp)), "rt_nw_render_denoised")
        else:
            check(load().rt_nw_render_adaptive(*args), "rt_nw_render_adaptive")
        self._adapt_shape = (H, W)
        if stats is not None:
            stats.update(passes=st.passes, stopped=st.stopped, total_samples=st.total_samples, pixels_at_max=st.pixels_at_max,
                         samples=st.samples, segments=st.segments, active=[int(v) for v in log[:min(st.passes, log.size)]])
        if raised:
            raise raised[0]
        return (mean, n, err, filtered) if denoise else (mean, n, err)

    def debug_trace(self, cam, W, H, i, j, s, max_depth=50, seed=1984, cap=64, with_time=False):
        """The segments of one camera sample: rows (o.xyz, d.xyz, t, n.xyz) and (winner index, box face);
        with_time: and the sample's ray time (rt_nw_debug_trace_t)."""
        rec = np.zeros(12 * cap, np.float32)
        n = C.c_int32()
        tm = C.c_float()
        if with_time:
            check(load().rt_nw_debug_trace_t(self._h, C.byref(cam), W, H, max_depth, seed, i, j, s, rec.ctypes.data_as(_fp),
                                             cap, C.byref(n), C.byref(tm)), "rt_nw_debug_trace_t")
        else:
            check(load().rt_nw_debug_trace(self._h, C.byref(cam), W, H, max_depth, seed, i, j, s, rec.ctypes.data_as(_fp),
                                           cap, C.byref(n)), "rt_nw_debug_trace")
        out = rec[: 12 * n.value].reshape(-1, 12).copy()
        segs = out[:, [0, 1, 2, 3, 4, 5, 6, 8, 9, 10]], out[:, [7, 11]].view(np.int32)
        return (*segs, np.float32(tm.value)) if with_time else segs

    def debug_hits(self, rays, keys=None):
        """Closest hit of each ray (rows o.xyz, d.xyz, time) through the walk
        this context renders with: (insertion index or -1, t, box face)."""
        n = len(rays)
        r = np.zeros((n, 8), np.float32)
        r[:, :7] = rays
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        idx, t, face = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.int32)
        check(load().rt_nw_debug_hits(self._h, r.ctypes.data_as(_fp),
                                      None if k is None else k.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                                      idx.ctypes.data_as(_ip), t.ctypes.data_as(_fp), face.ctypes.data_as(_ip)),
              "rt_nw_debug_hits")
        return idx, t, face

    def debug_records(self, rays, keys=None):
        """The hit record of each ray (rows o.xyz, d.xyz, time) as a render
        makes it (rt_nw_debug_records): (insertion index or -1, t, rows p.xyz
        n.xyz u v, material)."""
        n = len(rays)
        r = np.zeros((n, 8), np.float32)
        r[:, :7] = np.asarray(rays)[:, :7]
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        idx, t = np.zeros(n, np.int32), np.zeros(n, np.float32)
        rec, mat = np.zeros((n, 8), np.float32), np.zeros(n, np.int32)
        check(load().rt_nw_debug_records(self._h, r.ctypes.data_as(_fp),
                                         None if k is None else k.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                                         idx.ctypes.data_as(_ip), t.ctypes.data_as(_fp), rec.ctypes.data_as(_fp),
                                         mat.ctypes.data_as(_ip)), "rt_nw_debug_records")
        return idx, t, rec, mat

    def last_segments(self):
        v = C.c_uint64()
        check(load().rt_nw_ctx_last_segments(self._h, C.byref(v)), "rt_nw_ctx_last_segments")
        return v.value

    def scene_tri(self):
        """Diagnostic: the kernel family of the resident scene, 0..5 (rt_nw_ctx_scene_tri)."""
        v = C.c_int32()
        check(load().rt_nw_ctx_scene_tri(self._h, C.byref(v)), "rt_nw_ctx_scene_tri")
        return v.value

    def last_kernel(self):
        """Diagnostic: the last render's kernel (rt_nw_ctx_last_kernel)."""
        v = (C.c_int32 * 4)()
        check(load().rt_nw_ctx_last_kernel(self._h, v), "rt_nw_ctx_last_kernel")
        return dict(zip(("persistent", "grid", "spheres_only", "chunk"), list(v)))

    def last_staging(self):
        """Diagnostic: what the last render walked from LDS (rt_nw_ctx_last_staging)."""
        v = (C.c_int32 * 2)()
        check(load().rt_nw_ctx_last_staging(self._h, v), "rt_nw_ctx_last_staging")
        return {"nodes_lds": bool(v[0]), "objects_lds": bool(v[1])}

    def close(self):
        if self._h:
            load().rt_nw_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
