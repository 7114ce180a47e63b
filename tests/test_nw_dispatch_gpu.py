"""The Next-Week launch path (rtmi_nw.hip: one kernel table for query and
launch): every kernel family under every kernel shape a small scene reaches and
each of the four forms of a launch gives the same image, bit for bit.

  * families: one scene per has_tri 0 .. 5 — a preset, flat triangles among every
    other object kind, triangles with attribute records, and a shared mesh placed
    statically, with a move, and with an affine map;
  * shapes: RTMI_NW_PERSIST 1 and 0 (the persistent and the one-shot kernels), the
    BVH and — families 0 .. 2 — the uniform grid; family 0 also with the
    spheres-only instantiation turned off (the general persistent grid kernel);
  * forms: a render with all samples in one work item per tile (RTMI_NW_CHUNK =
    spp: the kernels that write floats), a chunked render (RTMI_NW_CHUNK = 4),
    a progressive pass and an adaptive pass with every pixel active.

36 x 20 pixels, 6 samples: neither side is a multiple of the 8 x 8 tile and the
second chunk of a tile holds 2 of 4 samples, the two places where a wrong item
count or a wrong number of blocks shows.  The staging rungs that need a scene too
large for LDS are reached by the tests of the families (test_nw_affine_gpu.py,
test_nw_smooth_gpu.py, test_nw_mesh_gpu.py, test_nw_mesh_oracle_gpu.py,
test_nw_motion_gpu.py); the six that none of them names — nodes in LDS and
objects in global memory under a persistent block for families 0, 3, 4 and 5,
and family 0's two one-shot rungs without the objects — are reached here by the
same scenes among 30 x 30 or 50 x 50 small spheres."""
import numpy as np
import pytest

import a_dive_into_ray_tracing_amd.nextweek as nw
import nw_affine_util as AU
import nw_mesh_util as M
import nw_mixed_util as X
import nw_motion_util as V
import nw_smooth_util as SU

pytestmark = pytest.mark.gpu
SEED = 1984
W, H, SPP, DEPTH, CHUNK = 36, 20, 6, 8, 4
GRID_LDS = {"nodes_lds": False, "objects_lds": True}  # the grid kernels stage the objects with the cells
ALL_LDS = {"nodes_lds": True, "objects_lds": True}
NODES_LDS = {"nodes_lds": True, "objects_lds": False}
NO_LDS = {"nodes_lds": False, "objects_lds": False}


def _mesh_cam():
    return nw.camera((6, 2.5, 7), M.CENTRE, (0, 1, 0), 35, W / H, 0.0, 9.0, 0.0, 1.0)


def _flat_mixed():
    """Family 1: every object kind (media, a rotated group, moving spheres) and a flat icosphere(1)."""
    def mesh(s):
        v, f = M.icosphere(1)
        s.add(s.mesh(v, f, mat=s.lambertian(s.solid(0.6, 0.5, 0.4))))
    return X.mixed_scene(mesh_only=mesh), X.mixed_camera(W, H)


def _crowd(s, side):
    """side x side small spheres among the scene's objects: 30 x 30 (about 610 BVH nodes, 900 objects) leave room
    in LDS for the nodes but not for the objects beside them, in a persistent block as in a one-shot one; 50 x 50
    (1 680 nodes, 54 KB; 2 500 objects, 130 KB) fit a persistent block's nodes alone and nothing of a one-shot block."""
    m = s.lambertian(s.solid(0.3, 0.6, 0.8))
    for i in range(side):
        for k in range(side):
            s.add(s.sphere((-6 + 12 * i / (side - 1), -3.0 + 0.3 * ((i + k) % 3), -5 + 12 * k / (side - 1)), 0.12, m))
    return s


def _spheres(side):
    s = nw.Scene()
    s.add(s.sphere((0, -1002, 0), 1000, s.lambertian(s.checker(s.solid(0.2, 0.3, 0.1), s.solid(0.9, 0.9, 0.9)))))
    s.add(s.sphere(M.CENTRE, 1.2, s.dielectric(1.5)))
    s.set_background(0.7, 0.8, 1.0)
    return _crowd(s, side)


_CAM5 = ((2.0, 4.5, 15.0), (0.4, 0.4, 1.4), (0, 1, 0), 40, W / H, 0.0, 10.0, 0.0, 1.0)
SCENES = {  # name: (family, builder of (scene, camera))
    "tri0": (0, lambda: nw.preset(2, aspect=W / H)),
    "tri1": (1, _flat_mixed),
    "tri2": (2, lambda: (SU.smooth_scene(subdiv=1, ground=True), _mesh_cam())),
    "tri3": (3, lambda: (V.scene_m("end0"), _mesh_cam())),
    "tri4": (4, lambda: (V.scene_m("moving"), _mesh_cam())),
    "tri5": (5, lambda: (AU.scene_a().scene, nw.camera(*_CAM5))),
    # the staging rungs no other test names for these families, at the smallest crowd that reaches them
    "tri0_crowd30": (0, lambda: (_spheres(30), _mesh_cam())),
    "tri0_crowd50": (0, lambda: (_spheres(50), _mesh_cam())),
    "tri3_crowd50": (3, lambda: (_crowd(V.scene_m("end0"), 50), _mesh_cam())),
    "tri4_crowd50": (4, lambda: (_crowd(V.scene_m("moving"), 50), _mesh_cam())),
    "tri5_crowd50": (5, lambda: (_crowd(AU.scene_a().scene, 50), nw.camera(*_CAM5))),
}
_SCENES, _REF = {}, {}


def _scene(name):
    if name not in _SCENES:
        _SCENES[name] = SCENES[name][1]()
    return _SCENES[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _reference(name):
    """(image, world.hit calls) of the scene under the default shape: rendered once, never changed."""
    if name not in _REF:
        s, cam = _scene(name)
        r = nw.NwRenderer(s)
        try:
            assert r.scene_tri() == SCENES[name][0]
            img = r.render(cam, W, H, SPP, DEPTH, SEED)
            segs = r.last_segments()
        finally:
            r.close()
        assert np.isfinite(img).all() and len(np.unique(img.reshape(-1, 3), axis=0)) > 20
        img.setflags(write=False)
        _REF[name] = (img, segs)
    return _REF[name]


# (scene, RTMI_NW_PERSIST, structure, the spheres-only instantiation allowed, what the launch stages)
SHAPES = [(f"tri{f}", p, a, True, GRID_LDS if a == "grid" else ALL_LDS)
          for f in range(6) for p in (1, 0) for a in (("bvh", "grid") if f < 3 else ("bvh",))]
SHAPES += [("tri0", 1, "grid", False, GRID_LDS)]  # the general persistent grid kernel of family 0
SHAPES += [("tri0_crowd30", 1, "bvh", True, NODES_LDS), ("tri0_crowd30", 0, "bvh", True, NODES_LDS),
           ("tri0_crowd50", 0, "bvh", True, NO_LDS)]
SHAPES += [(f"tri{f}_crowd50", 1, "bvh", True, NODES_LDS) for f in (3, 4, 5)]


@pytest.mark.parametrize("name,persist,accel,simple_ok,staging", SHAPES,
                         ids=[f"{n}-{'persistent' if p else 'one_shot'}-{a}{'' if s else '-general'}" for n, p, a, s, _ in SHAPES])
def test_forms_and_shapes_give_one_image(name, persist, accel, simple_ok, staging, monkeypatch):
    family = SCENES[name][0]
    want, want_segs = _reference(name)
    s, cam = _scene(name)
    monkeypatch.setenv("RTMI_NW_PERSIST", str(persist))  # (the three are read when a context is created)
    monkeypatch.setenv("RTMI_NW_SIMPLE", "1" if simple_ok else "0")
    kernel = {"persistent": persist, "grid": int(accel == "grid"),
              "spheres_only": int(family == 0 and accel == "grid" and persist == 1 and simple_ok)}

    def ctx(chunk):
        monkeypatch.setenv("RTMI_NW_CHUNK", str(chunk))
        r = nw.NwRenderer(s)
        r.set_accel(accel)
        assert r.scene_tri() == family and r.accel_info()["accel"] == accel, (r.scene_tri(), r.accel_info())
        return r

    def ran(r, chunk, what):
        k, st, segs = r.last_kernel(), r.last_staging(), r.last_segments()
        print(f"{name} persist {persist} {accel} {what}: {k} {st} segments {segs}")
        assert k == dict(kernel, chunk=chunk) and st == staging, (what, k, st)
        assert segs == want_segs, (what, segs, want_segs)

    r = ctx(SPP)  # one work item per tile: the kernels that write the floats themselves
    try:
        one = r.render(cam, W, H, SPP, DEPTH, SEED)
        ran(r, SPP, "one item per tile")
    finally:
        r.close()
    r = ctx(CHUNK)  # two items per tile, the second with 2 of 4 samples
    try:
        chunked = r.render(cam, W, H, SPP, DEPTH, SEED)
        ran(r, CHUNK, "chunked")
        r.accum_reset(W, H)
        r.render_pass(cam, W, H, 0, SPP, DEPTH, SEED)
        ran(r, CHUNK, "progressive pass")
        sums, done = r.accum_export()
        r.adapt_reset(W, H)
        r.adapt_pass(cam, W, H, SPP, DEPTH, SEED)
        ran(r, CHUNK, "adaptive pass")
        asum, _, an = r.adapt_export()
    finally:
        r.close()
    assert np.array_equal(_bits(one), _bits(want)) and np.array_equal(_bits(chunked), _bits(want))
    assert done == SPP and (an == SPP).all()
    assert np.array_equal(asum, sums)
    assert np.array_equal(_bits(sums.astype(np.float32) * np.float32(2.0 ** -32)), _bits(want))
