"""Shared pieces of tests/test_nw_instance.py and tests/test_nw_instance_gpu.py:
scenes that hold one mesh several times, built with Scene.shared (one pool of
triangles, one record per placement) or without it (today's flattened copies:
the reference of every comparison)."""
import numpy as np

import a_dive_into_ray_tracing_amd.nextweek as nw
import nw_mesh_util as M

# the four distinct placements of the five-placement scene (rotate_y degrees or
# None, translation or None); the fifth repeats the fourth
PLACEMENTS = [(None, None), (None, (3.1, 0.4, -0.7)), (30.0, None), (75.0, (-2.9, 0.3, 0.8))]
# spheres beside and inside the meshes (as test_nw_mesh_gpu.SPHERES)
SPHERES = [((2.5, 2.6, 0.9), 0.9), ((-1.9, -2.4, 0.9), 0.9), ((0.3, 2.0, 3.4), 0.8), ((0.3, -0.2, 0.9), 0.6)]


def place(s, h, rot, off):
    if rot is not None:
        h = s.rotate_y(h, rot)
    if off is not None:
        h = s.translate(h, off)
    return h


def five_placements(shared, subdiv=2, collinear=False, spheres=True):
    """icosphere(subdiv) placed five ways — identity, translate, rotate_y, both,
    and the last once more with the identical transform — plus spheres.
    collinear: one never-hit triangle joins the mesh."""
    s = nw.Scene()
    grey = s.lambertian(s.solid(0.6, 0.5, 0.4))
    v, f = M.icosphere(subdiv)
    mesh = s.mesh(v, f, mat=grey)
    if collinear:
        mesh = s.group([mesh, s.triangle((0, 0, 0), (1, 1, 1), (2, 2, 2), grey)])
    h = s.shared(mesh) if shared else mesh
    for rot, off in PLACEMENTS + PLACEMENTS[-1:]:
        s.add(place(s, h, rot, off))
    if spheres:
        sm = [grey, s.metal(s.solid(0.7, 0.6, 0.5), 0.0), s.dielectric(1.5), s.lambertian(s.solid(0.9, 0.2, 0.2))]
        for (c, r), m in zip(SPHERES, sm):
            s.add(s.sphere(c, r, m))
    s.set_background(0.7, 0.8, 1.0)
    return s


def field(shared, subdiv, n, spacing=4.0):
    """icosphere(subdiv) placed n times on a line-by-line field, each copy with
    its own rotate_y angle and translation (the first: no transform at all)."""
    s = nw.Scene()
    v, f = M.icosphere(subdiv)
    mesh = s.mesh(v, f, mat=s.lambertian(s.solid(0.6, 0.5, 0.4)))
    h = s.shared(mesh) if shared else mesh
    side = int(np.ceil(np.sqrt(n)))
    for q in range(n):
        i, k = divmod(q, side)
        s.add(h if q == 0 else place(s, h, 23.0 * q, (spacing * i, 0.25 * (q % 3), spacing * k)))
    s.set_background(0.7, 0.8, 1.0)
    return s


def mixed_placements(shared, mats="mixed"):
    """The material mix of test_nw_mesh_gpu.scene_a (lambertian, metal,
    dielectric and an image-textured lambertian — or a light — by quarters of
    icosphere(2)) placed three times over a ground sphere, two spheres beside."""
    s = nw.Scene()
    grey = s.lambertian(s.solid(0.6, 0.5, 0.4))
    v, f = M.icosphere(2)
    img = np.random.default_rng(5).integers(0, 256, (8, 8, 3)).astype(np.uint8)
    last = s.diffuse_light(s.solid(4, 4, 3)) if mats == "light" else s.lambertian(s.image(img))
    ms = [grey, s.metal(s.solid(0.8, 0.8, 0.9), 0.3), s.dielectric(1.5), last]
    q = len(f) // 4
    mesh = s.group([s.mesh(v, f[k * q:(k + 1) * q], mat=ms[k]) for k in range(4)])
    h = s.shared(mesh) if shared else mesh
    for rot, off in ((None, None), (30.0, (3.3, 0.3, -0.5)), (-50.0, (-3.4, 0.1, 0.6))):
        s.add(place(s, h, rot, off))
    s.add(s.sphere((0.3, -0.2, 0.9), 0.6, s.lambertian(s.solid(0.9, 0.2, 0.2))))  # inside the first mesh
    s.add(s.sphere((1.8, -1.2, 3.4), 0.7, s.dielectric(1.5)))
    s.add(s.sphere((0, -1002, 0), 1000, s.lambertian(s.checker(s.solid(0.2, 0.3, 0.1), s.solid(0.9, 0.9, 0.9)))))
    s.set_background(0.7, 0.8, 1.0)
    return s


def placement_of(flat_index, first, count):
    """Per flattened index the placement whose range [first[p], first[p] + count) holds it, or -1."""
    idx = np.asarray(flat_index)
    out = np.full(idx.shape, -1, np.int64)
    for p, f0 in enumerate(first):
        out[(idx >= f0) & (idx < f0 + count)] = p
    return out
