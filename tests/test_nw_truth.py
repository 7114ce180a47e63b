"""The Next-Week oracle (oracle/rt_nw_oracle.inc, what the kernels equal bit
for bit) against an independent float64 model of the reference's semantics
(tests/nw_truth.py) — every non-triangle kind: closest hits, hit records,
textures through emission, whole paths with their scatter relations and
colours, and the statistics of participating media.  Runs without a GPU;
tests/test_nw_truth_gpu.py holds the kernels to the same model.

Tolerances are formed, not chosen: 8 x the largest deviation of the model's
own float32 evaluation from its float64 evaluation on the kept inputs (per
winning object), conditions on their size asserted.  Every comparison is
shown to fail under a deliberate misreading of the reference (nw_truth.SWITCHES).
"""
import numpy as np
import pytest

import nw_truth as T
import oracle_py as O
from a_dive_into_ray_tracing_amd import nextweek as nw

W, H = 24, 16
INSTANT = 0.5  # the path scenes' shutter is one instant, so every segment's time is known


class Oracle:
    """The output under test: the oracle's debug entry points over one scene."""

    def __init__(self, scene):
        self.flat = scene.flat()

    def hits(self, rays, keys=None):
        return O.nw_hits(self.flat, rays, keys)

    def records(self, rays):
        return O.nw_records(self.flat, rays)

    def traces(self, cam, depth):
        return [O.nw_trace(self.flat, cam, W, H, depth, T.SEED, i, j, 0) for j in range(H) for i in range(W)]

    def image(self, cam, depth):
        return O.nw_render(self.flat, cam, W, H, 1, depth, T.SEED)[0]


class Case:
    """A scene, its model view, its rays and what was traced of it (cached per module)."""


@pytest.fixture(scope="module")
def t1():
    c = Case()
    c.scene, c.objs = T.scene_t1(nw)
    c.F = T.Flat(c.scene.flat())
    c.rays = T.rays_t1(c.objs)
    c.dev = Oracle(c.scene)
    c.hits = c.dev.hits(c.rays)
    c.records = c.dev.records(c.rays)
    c.paths = {}
    assert min(c.scene.grid_stats()["dims"]) >= 1  # (the GPU file walks T1's uniform grid and its BVH)
    return c


@pytest.fixture(scope="module")
def paths():
    c = Case()
    c.scene, c.cam = T.scene_paths(nw, W, H, INSTANT)
    c.F = T.Flat(c.scene.flat())
    c.dev = Oracle(c.scene)
    c.paths = {}
    return c


def traced(c, depth):
    if depth not in c.paths:
        c.paths[depth] = (c.dev.traces(c.cam, depth), c.dev.image(c.cam, depth))
    return c.paths[depth]


def check_path_coverage(cov, depth):
    """Both dielectric branches, every scattering material's relation on at
    least ten segments, and the ends a depth shows."""
    assert cov["branches"] == {"reflect", "refract"}, cov
    for m in (T.LAMBERTIAN, T.METAL, T.DIELECTRIC, T.ISOTROPIC):
        assert cov["relations"].get(m, 0) >= 10, cov
    assert cov["ends"]["miss"] > 0 and cov["ends"]["light" if depth == 50 else "limit"] > 0, cov


@pytest.fixture(scope="module")
def lights():
    c = Case()
    c.scene, c.cam = T.scene_lights(nw)
    c.F = T.Flat(c.scene.flat())
    c.dev = Oracle(c.scene)
    tr = c.dev.traces(c.cam, 50)
    c.rays = np.array([np.concatenate([t[0][0, 0:6], [INSTANT]]) for t in tr], np.float32)
    c.pixels = c.dev.image(c.cam, 50).reshape(-1, 3)
    return c


# ---- the model itself ------------------------------------------------------
def test_sphere_uv_worked_examples():
    """The six worked examples in the comment of get_sphere_uv (sphere.h:32-34)."""
    p = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    u, v = T.sphere_uv(p)
    want = np.array([[0.5, 0.5], [0.0, 0.5], [0.5, 1.0], [0.5, 0.0], [0.25, 0.5], [0.75, 0.5]])
    # <-1 0 0> is the seam: atan2(-0, -1) + pi is 0 or 2 pi, u 0 or 1
    assert np.abs(v - want[:, 1]).max() < 1e-15
    du = np.abs(u - want[:, 0])
    assert np.minimum(du, 1 - du).max() < 1e-15, u
    with pytest.raises(AssertionError):
        u2, _ = T.sphere_uv(p, sw=("phi_no_pi",))
        assert np.abs(u2 - want[:, 0])[[0, 4, 5]].max() < 1e-15


def test_flat_instances_are_the_float64_composition(t1):
    """translate and rotate_y in both nestings flatten to world = R local + off
    with the rotation of the summed angle: the flat view the model reads equals
    the float64 composition of the builder calls to float32 rounding."""
    F = t1.F
    for k, ob in enumerate(t1.objs):
        if not ob["chain"]:
            assert F.inst_of[k] < 0
            continue
        row = F.inst[F.inst_of[k]].astype(np.float64)
        angle = sum(a for op, a in ob["chain"] if op == "r")
        off = T._place((0, 0, 0), ob["chain"])
        assert abs(row[0] - np.cos(np.radians(angle))) < 1e-7 and abs(row[1] - np.sin(np.radians(angle))) < 1e-7, (k, row)
        assert np.abs(row[2:5] - off).max() < 1e-6, (k, row, off)
        # (the model's frame maps the local centre to where the builder calls put it)
        fr = T._frame(F, k, np.float64, ())
        local = T._place(ob["centre"], [(op, -a if op == "r" else -np.asarray(a)) for op, a in reversed(ob["chain"])])
        assert np.abs(T.point_to_world(fr, local[None], ())[0] - ob["centre"]).max() < 1e-6


# ---- the oracle against the model -------------------------------------------
def test_closest_hits(t1):
    """20 000 rays of scene T1: the same winner and box face on kept rays, t
    within 8 x the model's float32 deviation.  Seen on the CPU: formed relative
    tolerance of t 2.8e-4 (the R = 1000 sphere; <= 1e-3 required), largest
    error 5.0e-5; the filters drop 0.4 % of the model's hits."""
    cov, rep = {}, {}
    T.compare_hits(t1.F, t1.rays, t1.hits, coverage=cov, report=rep)
    T.check_coverage(t1.F, cov)
    assert {0, 1} == set(np.unique(cov["root"][cov["kept"] & np.isin(cov["idx"], (2, 3))]).tolist())  # the glass shells
    print("hits", rep, "dropped", cov["dropped"])


def test_misses_stay_misses(t1):
    """Kept rays the model sees miss everything miss in the oracle too (covered
    by the winner comparison: -1 is a winner), and there are some."""
    h64, _, _, keep = T.model_hits(t1.F, t1.rays)
    miss = keep & (h64["idx"] < 0)
    assert miss.sum() >= 100
    assert (np.asarray(t1.hits[0])[miss] == -1).all()


def test_hit_records(t1):
    """p, n, u, v and the material of the same rays.  Seen on the CPU (formed
    tolerance / largest error): p relative 9.3e-4 / 8.9e-5, n 3.6e-5 / 3.6e-6,
    u 1.1e-5 / 1.5e-6, v 4.5e-5 / 5.6e-6 (n, u, v of a sphere where its
    conditioning number nw_truth.KAPPA_MAX allows)."""
    rep = {}
    T.compare_records(t1.F, t1.rays, t1.records, report=rep)
    print("records", rep)


def test_textures_through_emission(lights):
    """A scene of diffuse_light(texture) objects — image on a sphere, marble,
    checker over an image on a rect, the null image on a placed box, a solid
    checker, a solid — at 1 spp on black: each pixel is the model's texture
    value at the model's record of the camera ray.  Seen on the CPU: formed
    tolerance 6.5e-4 (the marble; <= 1e-3 required), largest error 7.4e-5."""
    rep = {}
    T.compare_emission(lights.F, lights.rays, lights.pixels, report=rep)
    print("emission", rep)


@pytest.mark.parametrize("depth", [50, 3])
def test_whole_paths(paths, depth):
    """Every pixel's sample 0 of a 24 x 16 image of the path scene (every kind
    and material, large spheres near the camera) on a non-black background:
    per segment the winner, t, n and the scatter relation into the next
    segment, a metal's ending both ways; the 1-spp pixel is the model's path
    colour.  Seen on the CPU at depth 50 (formed tolerance / largest error): t
    7.7e-4 / 9.6e-5, n 2.7e-5 / 2.8e-6, o' = p 5.2e-4 / 6.4e-5, the mirror
    direction 6.5e-5 / 7.9e-6, the dielectric directions 3.8e-5 / 3.7e-6,
    colour 1.7e-4 / 2.0e-5.  The filters, KAPPA_MAX included, drop 3.6 % of the
    hit segments and 3.7 % of the scatter pairs (depth 3: 3.2 %, 3.5 %); 368 of
    384 colours are compared (377), none dropped for a texture jump; relations
    checked: lambertian 363, metal 90, dielectric 369, isotropic 115 (243, 71,
    141, 65); 6 absorbed mirror hits checked (2); at depth 3, 139 paths end at
    the limit."""
    traces, image = traced(paths, depth)
    rep, cov = {}, {}
    T.compare_paths(paths.F, traces, image, depth, INSTANT, report=rep, coverage=cov)
    print("paths", depth, rep, cov)
    check_path_coverage(cov, depth)


# ---- media -------------------------------------------------------------------
MEDIA = [("sphere", 1, False), ("box", 1, False), ("sphere", 2, False), ("box", 2, False), ("sphere", 1, True)]


def medium_case(which, samples, glass):
    s, centre, size = T.scene_medium(nw, which, samples, glass)
    rays, keys = T.rays_medium(centre, size)
    return s, T.Flat(s.flat()), rays, keys


@pytest.mark.parametrize("which,samples,glass", MEDIA)
def test_medium_statistics(which, samples, glass):
    """A medium alone in its scene, 20 000 rays with random keys: hits lie in
    the float64 span of the boundary, their number within |z| <= 5 of the
    expectation, and (samples = 1) the conditional position is uniform.  With
    the boundary also in the world as glass the hit probability is the same:
    the medium hides its own boundary.  Seen on the CPU: |z| <= 0.81 over the
    five cases, sqrt(n) D_KS 0.52 (sphere) and 0.46 (box)."""
    s, F, rays, keys = medium_case(which, samples, glass)
    rep = {}
    T.check_medium(F, rays, Oracle(s).hits(rays, keys), samples, full=not glass, report=rep)
    print("medium", which, samples, glass, rep)


# ---- sensitivity: every comparison fails under a misreading --------------------
def test_misread_transforms_fail_hits_and_records(t1):
    for sw in ("rotate_sign", "instance_order"):
        with pytest.raises(T.Mismatch):
            T.compare_hits(t1.F, t1.rays, t1.hits, sw=(sw,))
        with pytest.raises(T.Mismatch):
            T.compare_records(t1.F, t1.rays, t1.records, sw=(sw,))


def test_misread_phi_fails_records(t1):
    with pytest.raises(T.Mismatch, match="records u"):
        T.compare_records(t1.F, t1.rays, t1.records, sw=("phi_no_pi",))


@pytest.mark.parametrize("sw", ["perlin_unsmoothed_offsets", "phi_no_pi", "image_no_shift", "image_no_flip"])
def test_misread_textures_fail_emission(lights, sw):
    with pytest.raises(T.Mismatch, match="emission"):
        T.compare_emission(lights.F, lights.rays, lights.pixels, sw=(sw,))


def test_misread_dielectric_fails_paths(paths):
    traces, image = traced(paths, 50)
    with pytest.raises(T.Mismatch, match="dielectric"):
        T.compare_paths(paths.F, traces, image, 50, INSTANT, sw=("dielectric_reflect_unit",))


def test_misread_depth_limit_fails_paths(paths):
    traces, image = traced(paths, 3)
    with pytest.raises(T.Mismatch, match="colour"):
        T.compare_paths(paths.F, traces, image, 3, INSTANT, sw=("depth_limit_attenuated",))


def tangent_case():
    """sphere (0, 0, 0) r 1 and the ray (-2, 1, 0) + t (1, 0, 0): a = 1, b = -2,
    c = 4, disc = 0 exactly in float and in double.  sphere::hit wants disc > 0."""
    s = nw.Scene()
    s.add(s.sphere((0, 0, 0), 1.0, s.lambertian(s.solid(0.5, 0.5, 0.5))))
    return s, np.array([[-2, 1, 0, 1, 0, 0, 0]], np.float32)


def edge_case():
    """box (0, 0, 0)-(1, 1, 1) and the ray (0.5, 2, 2) + t (0, -1, -1): it meets
    the edge y = z = 1 at t = 1 on side 0 (z = 1) and side 2 (y = 1), every
    number exact; the later side of box.h's list wins the tie."""
    s = nw.Scene()
    s.add(s.box((0, 0, 0), (1, 1, 1), s.lambertian(s.solid(0.5, 0.5, 0.5))))
    return s, np.array([[0.5, 2, 2, 0, -1, -1, 0]], np.float32)


def constructed(make, dev_of):
    s, rays = make()
    F = T.Flat(s.flat())
    return F, rays, dev_of(s).hits(rays)


def check_constructed(make, dev_of, switch, want):
    """The exact case: the output under test equals the model, and differs from its misreading."""
    F, rays, (idx, t, face) = constructed(make, dev_of)
    h = T.closest_hit(F, rays)
    assert (int(h["idx"][0]), int(h["face"][0])) == want[:2] and (want[2] is None or h["t"][0] == want[2])
    if (int(idx[0]), int(face[0])) != want[:2] or (want[2] is not None and float(t[0]) != want[2]):
        raise T.Mismatch(f"{make.__name__}: model {want}, device ({idx[0]}, {face[0]}, {t[0]})")
    m = T.closest_hit(F, rays, sw=(switch,))
    assert (int(m["idx"][0]), int(m["face"][0])) != want[:2], "the misreading changes nothing"


def test_exact_tangent_ray_misses_the_open_sphere():
    check_constructed(tangent_case, Oracle, "sphere_closed", (-1, -1, None))


def test_box_edge_goes_to_the_later_side():
    check_constructed(edge_case, Oracle, "box_tie_earlier", (0, 2, 1.0))
