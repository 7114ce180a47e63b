"""Shared pieces of tests/test_nw_mesh_oracle_gpu.py: the mixed scene — every
object kind of the Next-Week renderer beside triangle meshes — its cameras,
and the oracle side of a comparison (image, segment count and the winners by
kind, rendered once per case and kept)."""
import numpy as np

import a_dive_into_ray_tracing_amd.nextweek as nw
import nw_mesh_util as M
import nw_smooth_util as S
import oracle_py as O

SEED = 1984
ROT, OFF = 30.0, (4.6, 0.3, -1.6)  # the icosphere's second placement
LIGHT_CENTRE, LIGHT_RADIUS = (-2.4, 1.6, 3.0), 0.55
GLASS_QUARTER = 2  # the quarter of the icosphere's faces that is dielectric


def _perlin_tables(seed):
    g = np.random.default_rng(seed)
    return g.uniform(-1, 1, (256, 3)).astype(np.float32), np.stack([g.permutation(256) for _ in range(3)]).astype(np.int32)


def _mesh(s, v, f, mat, attr, centre, radius, flags=3):
    """One mesh part; attr: the sphere's normals and the affine uvs at its
    corners (flags 3), or an attribute call with flags 0."""
    if not attr:
        return s.mesh(v, f, mat=mat)
    nrm, uv = S.sphere_normals(v, centre, radius), S.affine_uvs(v)
    if flags == 0:
        return s.mesh_attr(np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.int32), np.ascontiguousarray(nrm),
                           None, None, None, 0, mat)
    return s.mesh(v, f, normals=nrm, uvs=uv, smooth=True, mat=mat)


def mixed_scene(shared=False, attr=False, second_subdiv=2, mesh_only=None):
    """Every object kind at once (the model: tests/test_nw_gpu.py::
    test_grid_mixed_objects_bit_exact) around an icosphere(2) in four
    material quarters — lambertian, metal with fuzz, dielectric, image-textured
    lambertian — that stands once in place and once under rotate_y + translate;
    a small mesh of emitting triangles; one collinear triangle (in the
    icosphere's group).  attr: the meshes carry sphere normals and affine uvs,
    the metal quarter an attribute call with flags 0.  shared: the icosphere is
    one Scene.shared handle placed three times, the last two with the
    identical transform (t ties between their copies).
    second_subdiv: the copy under rotate_y + translate is built from
    icosphere(second_subdiv) instead (fewer objects: the one-shot grid kernel's
    LDS); mesh_only: replaces the meshes by one call mesh_only(scene) (the
    staging tests)."""
    s = nw.Scene()
    solid = s.solid
    grey = s.lambertian(solid(0.6, 0.5, 0.4))
    red = s.lambertian(solid(0.8, 0.25, 0.2))
    steel = s.metal(solid(0.8, 0.8, 0.9), 0.3)
    mirror = s.metal(solid(0.7, 0.6, 0.5), 0.0)
    glass = s.dielectric(1.5)
    image = s.image(S.TEXTURE)
    mats = [grey, mirror, glass]
    # ground: a checker texture
    s.add(s.sphere((0, -1002, 0), 1000, s.lambertian(s.checker(solid(0.2, 0.3, 0.1), solid(0.9, 0.9, 0.9)))))
    # static spheres
    for k, (c, r) in enumerate([((3.0, -1.4, 4.6), 0.6), ((-0.9, -1.5, 5.6), 0.5), ((7.4, -1.3, 1.8), 0.7), ((1.9, 2.4, -2.6), 0.8),
                                ((-4.6, -1.2, 4.2), 0.8), ((0.3, -0.2, 0.9), 0.6)]):  # the last one inside the icosphere
        s.add(s.sphere(c, r, mats[k % 3]))
    # moving spheres: time ranges inside and outside the shutter (0.3, 0.6)
    ranges = [(0.0, 1.0), (0.2, 0.7), (-0.5, 0.5), (0.4, 2.0), (0.35, 0.55), (0.7, 0.9)]
    for k, (c, r) in enumerate([((1.2, -1.4, 6.6), 0.6), ((5.2, -1.3, 5.6), 0.7), ((-3.2, 0.6, -1.4), 0.8), ((8.2, 1.4, -2.4), 0.9),
                                ((-1.6, 2.6, -2.0), 0.7), ((3.4, 2.6, 1.6), 0.6)]):
        c1 = (c[0] + 0.5 - 0.25 * k, c[1] + 0.3 + 0.1 * k, c[2] + 0.2 * k - 0.4)
        s.add(s.moving_sphere(c, c1, *ranges[k], r, [red, steel, glass][k % 3]))
    # rectangles in the three planes, one of them a light
    s.add(s.rect("xy", -7.0, 11.0, -2.0, 6.5, -5.0, s.lambertian(solid(0.7, 0.7, 0.75))))
    s.add(s.rect("yz", -2.0, 6.5, -5.0, 9.0, -6.5, steel))
    s.add(s.rect("xz", -1.5, 4.5, -2.0, 4.0, 6.4, s.diffuse_light(solid(7, 7, 6))))
    s.add(s.rect("xz", 5.0, 8.0, 3.0, 6.0, -1.0, red))
    # boxes
    s.add(s.box((1.4, -2.0, 3.2), (2.4, -0.9, 4.2), red))
    s.add(s.box((-3.4, -2.0, 5.4), (-2.2, -0.4, 6.6), mirror))
    s.add(s.box((6.0, -2.0, -3.4), (7.6, 0.6, -1.8), glass))
    # a rotated and translated group of spheres and boxes (built about the origin)
    kids = [s.sphere((0.0, -1.3, 0.0), 0.7, steel), s.sphere((1.5, -0.2, 0.4), 0.5, glass),
            s.box((-1.8, -2.0, -0.6), (-0.8, 0.2, 0.6), grey), s.box((0.6, -2.0, 1.0), (1.8, -1.0, 2.2), red),
            s.moving_sphere((-0.4, 0.6, 1.4), (-0.2, 1.0, 1.6), 0.2, 0.7, 0.5, grey)]
    s.add(s.translate(s.rotate_y(s.group(kids), 25.0), (-3.4, 0.0, 0.6)))
    # media: a box-bounded and a moving-sphere-bounded one
    s.add(s.constant_medium(s.box((3.6, -2.0, 5.8), (5.6, 0.2, 7.6), grey), 0.9, solid(0.9, 0.9, 0.9)))
    s.add(s.constant_medium(s.moving_sphere((-0.6, -0.6, 7.2), (-0.4, -0.2, 7.5), 0.0, 1.0, 1.0, grey), 1.2, solid(0.3, 0.4, 0.8)))
    # a noise-textured and an image-textured sphere
    s.add(s.sphere((7.0, -1.0, 4.2), 1.0, s.lambertian(s.noise(4.0, *_perlin_tables(3)))))
    s.add(s.sphere((-2.0, -1.0, 3.4), 1.0, s.lambertian(image)))
    if mesh_only is not None:
        mesh_only(s)
    else:
        ms = [grey, steel, glass, s.lambertian(image)]

        def quarters(subdiv):
            v, f = M.icosphere(subdiv)
            q = len(f) // 4
            return [_mesh(s, v, f[k * q:(k + 1) * q], ms[k], attr, M.CENTRE, M.RADIUS, 0 if k == 1 else 3) for k in range(4)]

        mesh = s.group(quarters(2) + [s.triangle((0, 0, 0), (1, 1, 1), (2, 2, 2), grey)])  # (collinear: never hit)
        if shared:
            h = s.shared(mesh)
            s.add(h)
            s.add(s.translate(s.rotate_y(h, ROT), OFF))
            s.add(s.translate(s.rotate_y(h, ROT), OFF))
        else:
            s.add(mesh)
            s.add(s.translate(s.rotate_y(mesh if second_subdiv == 2 else s.group(quarters(second_subdiv)), ROT), OFF))
        lv, lf = M.icosphere(0, LIGHT_RADIUS, LIGHT_CENTRE)
        s.add(_mesh(s, lv, lf, s.diffuse_light(solid(4, 4, 3)), attr, LIGHT_CENTRE, LIGHT_RADIUS))
    s.set_background(0.7, 0.8, 1.0)
    return s


def mixed_camera(W, H, aperture=0.15, lookfrom=(5.5, 3.0, 12.5), lookat=(1.6, -0.2, 0.9), vfov=30.0):
    """Shutter (0.3, 0.6); aperture 0: a pinhole."""
    d = np.asarray(lookfrom, np.float64) - np.asarray(lookat, np.float64)
    return nw.camera(lookfrom, lookat, (0, 1, 0), vfov, W / H, aperture, float(np.sqrt((d * d).sum())), 0.3, 0.6)


INSIDE_LOOKAT = (2.0, -0.8, 7.0)  # between the two media


def inside_camera(W, H):
    """A pinhole inside the in-place icosphere, behind its dielectric quarter:
    at 0.8 of the way from the centre (beyond the sphere in the middle) to the
    centroid of the glass face that looks most directly at INSIDE_LOOKAT,
    looking there — at the media, the boxes and the spheres in front."""
    v, f = M.icosphere(2)
    q = len(f) // 4
    c = np.asarray(M.CENTRE)
    cen = v[f[GLASS_QUARTER * q:(GLASS_QUARTER + 1) * q]].mean(axis=1) - c
    d = np.asarray(INSIDE_LOOKAT) - c
    eye = c + 0.8 * cen[np.argmax(cen @ d / np.linalg.norm(cen, axis=1))]
    return nw.camera(tuple(eye), INSIDE_LOOKAT, (0, 1, 0), 70.0, W / H, 0.0, 1.0, 0.3, 0.6)


def shares(won):
    """(share of the hitting segments per kind group, share of misses among all segments)."""
    hit = sum(v for k, v in won.items() if k != "miss")
    rect = won["rect_xy"] + won["rect_xz"] + won["rect_yz"]
    g = {"triangle": won["triangle"], "moving_sphere": won["moving_sphere"], "rect": rect, "box": won["box"],
         "medium": won["medium"], "sphere": won["sphere"]}
    return {k: v / max(hit, 1) for k, v in g.items()}, won["miss"] / max(hit + won["miss"], 1)


def assert_mixed_conditions(won):
    """The conditions on the mixed scene, from the oracle's winners alone:
    triangles win at least 15% of the segments that hit something, moving
    spheres, rectangles, boxes and media at least 1% each, and at most 60% of
    all segments miss."""
    sh, miss = shares(won)
    assert sh["triangle"] >= 0.15, (sh, miss)
    for k in ("moving_sphere", "rect", "box", "medium"):
        assert sh[k] >= 0.01, (k, sh, miss)
    assert miss <= 0.60, (sh, miss)
    return sh, miss


_ORACLE = {}


def oracle_image(key, scene, cam, W, H, spp, depth=50, seed=SEED, **rows):
    """(image, segments, winners) of the oracle for a case, rendered once per key."""
    if key not in _ORACLE:
        _ORACLE[key] = O.nw_render(scene.flat(), cam, W, H, spp, depth, seed, flat_attr=scene.flat_attr(), winners=True, **rows)
    return _ORACLE[key]
