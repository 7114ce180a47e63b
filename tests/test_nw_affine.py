"""Affine placements of shared meshes (Scene.transform, rt_nw_transform) on the
CPU: what may stand under a transform node and which matrices it takes; the
composition of a placement's chain against numpy float64; the baked flat view;
the checker (tests/native/nw_affine_ref.cpp) against float64 ground truth, a
closed form for the normals and its watertightness; the host build under ASan +
UBSan (tests/native/nw_affine_sanitize.cpp); the CLI's argument check."""
import os
import subprocess

import numpy as np
import pytest

import nw_affine_util as AU
import nw_instance_util as U
import nw_mesh_util as M
import nw_motion_util as V
import nw_smooth_util as SU
from a_dive_into_ray_tracing_amd import _abi, nextweek as nw

REPO = M.REPO
CSRC = os.path.join(REPO, "a_dive_into_ray_tracing_amd", "csrc")
CLANG = "/opt/rocm/llvm/bin/clang++"
EINVAL, EUNSUPPORTED = -1, -4  # include/rtmi.h
SAN = ["-fsanitize=address", "-fsanitize=undefined", "-fno-sanitize-recover=all"]  # the Makefile's SAN
F32 = np.float32


def _code(fn):
    with pytest.raises(_abi.RTError) as e:
        fn()
    return e.value.code


def _diag(*d):
    return np.concatenate([np.diag(np.asarray(d, np.float64)), np.zeros((3, 1))], axis=1)


# ---- 1. what can and cannot be transformed --------------------------------------------
def test_what_cannot_be_transformed():
    s = nw.Scene()
    mat = s.lambertian(s.solid(0.5, 0.5, 0.5))
    v, f = M.icosphere(0)
    mesh = s.mesh(v, f, mat=mat)
    h = s.shared(mesh)
    m = nw.affine(scale=(2, 0.5, 1), axis=(1, 1, 0), angle=33, translate=(1, 2, 3))
    a, b = (0, 0, 0), (1, 0, 0)
    # one shared handle under translate, rotate_y, transform and at most one move, in any order
    assert s.transform(h, m) >= 0 and s.transform(h, np.vstack([m, [0, 0, 0, 1]])) >= 0 and s.transform(h, m.tolist()) >= 0
    t1 = s.transform(s.translate(s.rotate_y(s.transform(h, m), 20), b), m)
    assert t1 >= 0 and s.transform(s.move(s.rotate_y(t1, 3), a, b), _diag(1, 2, 1)) >= 0
    with pytest.raises(ValueError):
        s.transform(h, np.vstack([m, [0, 0, 1, 1]]))
    with pytest.raises(ValueError):
        s.transform(h, np.eye(3))
    # the matrix
    assert _code(lambda: s.transform(h, _diag(-1, 1, 1))) == EINVAL  # a mirror
    assert _code(lambda: s.transform(h, _diag(-1, -1, -1))) == EINVAL
    assert _code(lambda: s.transform(h, _diag(1, 1, 0))) == EINVAL  # singular
    assert _code(lambda: s.transform(h, np.ones((3, 4)))) == EINVAL
    bad = m.copy()
    bad[1, 2] = np.nan
    assert _code(lambda: s.transform(h, bad)) == EINVAL
    bad[1, 2] = 1e39  # not finite as a float
    assert _code(lambda: s.transform(h, bad)) == EINVAL
    bad = m.copy()
    bad[2, 3] = np.inf
    assert _code(lambda: s.transform(h, bad)) == EINVAL
    assert _code(lambda: s.transform(h, _diag(64, 1 / 64, 1))) == EINVAL  # beyond the conditioning bound
    assert _code(lambda: s.transform(h, _diag(1e-3, 1, 1))) == EINVAL
    assert s.transform(h, _diag(16, 1 / 16, 1)) >= 0 and s.transform(h, _diag(16, 16, 16)) >= 0
    assert s.transform(h, _diag(1 / 16, 1 / 16, 1 / 16)) >= 0 and s.transform(h, _diag(16, 1 / 16, 1 / 16)) >= 0
    R = nw.affine(axis=(1, 2, 3), angle=77)[:, :3]
    assert s.transform(h, np.concatenate([R @ np.diag([16, 1 / 16, 1]) @ R.T, np.zeros((3, 1))], axis=1)) >= 0
    assert _code(lambda: s.transform(-1, m)) == EINVAL and _code(lambda: s.transform(10 ** 6, m)) == EINVAL
    # what stands under it
    sph = s.sphere((0, 0, 0), 1, mat)
    assert _code(lambda: s.transform(sph, m)) == EUNSUPPORTED  # a primitive
    assert _code(lambda: s.transform(mesh, m)) == EUNSUPPORTED  # a flattened mesh
    assert _code(lambda: s.transform(s.translate(mesh, b), m)) == EUNSUPPORTED
    assert _code(lambda: s.transform(s.group([h]), m)) == EUNSUPPORTED  # a group
    assert _code(lambda: s.transform(s.group([h, h]), m)) == EUNSUPPORTED
    assert _code(lambda: s.transform(s.constant_medium(sph, 0.1, s.solid(1, 1, 1)), m)) == EUNSUPPORTED
    tf = s.transform(h, m)
    assert _code(lambda: s.shared(tf)) == EUNSUPPORTED
    assert _code(lambda: s.constant_medium(tf, 0.1, s.solid(1, 1, 1))) == EUNSUPPORTED
    assert _code(lambda: s.constant_medium(s.translate(tf, b), 0.1, s.solid(1, 1, 1))) == EUNSUPPORTED
    # a move over a chain with transforms; one move per chain
    mv = s.move(s.rotate_y(tf, 5), a, b, 0.25, 0.75)
    assert mv >= 0
    assert _code(lambda: s.move(mv, a, b)) == EUNSUPPORTED
    assert _code(lambda: s.move(s.transform(mv, m), a, b)) == EUNSUPPORTED
    assert _code(lambda: s.move(s.transform(s.translate(mv, b), m), a, b)) == EUNSUPPORTED
    # the handle goes where a translate handle goes
    s.add(s.translate(s.group([tf, sph]), (0, 0, 2)))
    s.add(s.rotate_y(mv, 10))
    s.add(s.transform(s.move(h, a, b), m))
    s.add(s.move(s.rotate_y(h, 4), a, b))
    s.add(h)
    assert s.affine_stats() == (3, 2) and s.motion_stats() == (3, 2) and s.instancing_stats()["placements"] == 5


def test_a_composite_over_the_bound_is_refused_at_flatten():
    s = nw.Scene()
    v, f = M.icosphere(0)
    h = s.shared(s.mesh(v, f, mat=s.lambertian(s.solid(0.5, 0.5, 0.5))))
    s.add(s.transform(h, _diag(16, 1 / 16, 1)))
    assert s.affine_stats() == (1, 0) and s.flat()["n_obj"] == 20
    s.add(s.translate(h, (5, 0, 0)))
    s.add(s.transform(s.rotate_y(s.transform(h, _diag(16, 1 / 16, 1)), 90), _diag(1, 16, 1)))  # fine: singular values 16, 1, 1
    assert s.affine_stats() == (2, 1)
    s.add(s.transform(s.transform(h, _diag(16, 1 / 16, 1)), _diag(16, 1 / 16, 1)))  # 256, 1/256, 1
    for call in (s.flat, lambda: s.flat(time=0.5), s.flat_attr, s.affine_stats, s.motion_stats, s.instancing_stats, s.grid_stats):
        with pytest.raises(_abi.RTError) as e:
            call()
        assert e.value.code == EINVAL and "placement 3" in str(e.value), str(e.value)


# ---- 2. composition ---------------------------------------------------------------------
M1 = nw.affine(scale=(1.3, 0.7, 1.1), axis=(1, 2, -1), angle=51.0, translate=(0.4, -1.1, 2.2))
M2 = AU.shear(0.5, (2.0, 0.5, 1.0), (-3.0, 0.25, 0.5))
MV = ((0.3, 0.5, -0.4), (1.5, -0.2, 0.6), 0.25, 0.75)
CHAINS = [
    [("transform", M1)],
    [("translate", (1, 2, 3)), ("transform", M1), ("translate", (-0.5, 0.1, 0.7))],
    [("rotate_y", 33.0), ("transform", M2), ("rotate_y", -70.0)],
    [("move", *MV), ("transform", M1), ("transform", M2)],
    [("transform", M2), ("move", *MV), ("rotate_y", 15.0)],
    # each node type above and below a transform
    [("translate", (2, 0, -1)), ("rotate_y", 40.0), ("move", *MV), ("transform", M1), ("translate", (0.2, 0.3, 0.4)),
     ("rotate_y", -25.0), ("transform", M2)],
    [("rotate_y", 10.0), ("translate", (0, 1, 0)), ("transform", M2), ("rotate_y", 80.0), ("move", *MV), ("translate", (1, 1, 1))],
]


def _numpy_map(chain, T):
    """(A, b) of the chain at the instant T by 4 x 4 float64 products; the move's ends rounded to float32 and
    taken through off(T) as the specification says."""
    def mat4(A=np.eye(3), b=(0, 0, 0)):
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = A, b
        return m

    def total(move_off):
        m = np.eye(4)
        for node in chain:
            if node[0] == "translate":
                m = m @ mat4(b=node[1])
            elif node[0] == "rotate_y":
                th = np.radians(node[1])
                m = m @ mat4(np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]]))
            elif node[0] == "transform":
                m = m @ mat4(np.asarray(node[1])[:, :3], np.asarray(node[1])[:, 3])
            else:
                m = m @ mat4(b=node[move_off])
        return m

    mv = [n for n in chain if n[0] == "move"]
    if not mv:
        m = total(None)
        return m[:3, :3], m[:3, 3]
    m0, m1 = total(1), total(2)
    return m0[:3, :3], V.off_at(m0[:3, 3].astype(F32), m1[:3, 3].astype(F32), mv[0][3], mv[0][4], T).astype(np.float64)


@pytest.mark.parametrize("T", [0.0, 0.5, float(F32(1) / F32(3))])
def test_baked_vertices_equal_the_float64_composition(T):
    v, f = M.icosphere(1)
    pl = AU.placed(lambda s: s.mesh(v, f, mat=s.lambertian(s.solid(0.5, 0.5, 0.5))), CHAINS, 80)
    assert pl.affine == list(range(len(CHAINS))) and pl.scene.motion_stats() == (4, 3)
    obj, inst = M.flat_arrays(pl.scene.flat(time=T))
    assert len(obj) == 80 * len(CHAINS) and len(inst) == 0 and (obj[:, 14].view(np.int32) == -1).all()
    local = v[f]  # (the vertices are float32 values)
    for p, chain in enumerate(CHAINS):
        A, b = _numpy_map(chain, T)
        want = (local @ A.T + b).astype(F32)
        got = obj[80 * p:80 * (p + 1), :9].reshape(-1, 3, 3)
        ulp = np.spacing(np.abs(want)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        assert (err <= ulp).all(), (p, err.max(), (err / ulp).max())
        # ... and the util's own composition (the checker's table) is the same map
        A2, b2, b12, (t0, t1), _ = pl.comp[p]
        bT = b2 if b12 is None else V.off_at(b2.astype(F32), b12.astype(F32), t0, t1, T)
        assert np.abs(A2 - A).max() < 1e-13 and np.abs(bT - b).max() < 1e-6


def test_baked_normals_are_the_inverse_transpose():
    pl = AU.placed(AU.a_mesh, [[("transform", M2)], [("rotate_y", 12.0)]], 320)
    fa, loc = pl.scene.flat_attr(), pl.local
    assert len(fa["attr"]) == 2 * 320 and np.array_equal(fa["attr_of_obj"], np.concatenate([np.arange(320, 640), np.arange(320)]))
    assert fa["attr"][:320].tobytes() == loc["attr"].tobytes()
    n = loc["attr"][:, :9].astype(np.float64).reshape(-1, 3, 3) @ np.linalg.inv(M2[:, :3])  # rows n^T A^-1 = (A^-T n)^T
    n /= np.linalg.norm(n, axis=2)[:, :, None]
    assert np.abs(fa["attr"][320:, :9].reshape(-1, 3, 3) - n).max() < 1e-7
    assert fa["attr"][320:, 9:].tobytes() == loc["attr"][:, 9:].tobytes()  # uvs and flags as they are


def test_scenes_without_a_transform_are_unchanged():
    """The same scene with and without one more object — an affine placement of
    the shared mesh, added last: every row of the others is byte for byte what it was."""
    def build(extra):
        s = U.five_placements(True, spheres=False)
        v, f = M.icosphere(1)
        h = s.shared(s.mesh(v, f, normals=SU.sphere_normals(v), smooth=True, mat=s.lambertian(s.solid(0.2, 0.3, 0.4))))
        s.add(s.move(s.translate(s.rotate_y(h, 50), (0, 4, 0)), (0, 0, 0), (1, 0, 0)))
        s.add(s.sphere((9, 9, 9), 1.0, s.lambertian(s.solid(0.5, 0.5, 0.5))))
        if extra:
            s.add(s.transform(h, M1))
        return s

    a, b = build(False), build(True)
    assert a.affine_stats() == (0, 6) and b.affine_stats() == (1, 6)
    for T in (None, 0.7):
        fa, fb = a.flat(time=T), b.flat(time=T)
        n = fa["n_obj"]
        assert fb["n_obj"] == n + 80 and fb["obj"][:16 * n].tobytes() == fa["obj"].tobytes()
        assert [k for k in fa if k not in ("obj", "n_obj") and np.asarray(fa[k]).tobytes() != np.asarray(fb[k]).tobytes()] == []
    aa, ab = a.flat_attr(), b.flat_attr()
    assert ab["attr"][:len(aa["attr"])].tobytes() == aa["attr"].tobytes() and len(ab["attr"]) == len(aa["attr"]) + 80
    assert ab["attr_of_obj"][:len(aa["attr_of_obj"])].tobytes() == aa["attr_of_obj"].tobytes()
    sa, sb = a.instancing_stats(), b.instancing_stats()
    assert sb["placements"] == sa["placements"] + 1 and sb["top_leaves"] == sa["top_leaves"] + 1
    assert all(sa[k] == sb[k] for k in ("meshes", "pool_triangles", "bottom_nodes"))
    # without any transform node the flat view is still the flattened copies'
    assert V.flats_equal(U.five_placements(True).flat(), U.five_placements(False).flat()) is None


def test_flat_at_time_bakes_the_formula():
    chain = [("rotate_y", 10.0), ("move", *MV), ("transform", M1)]
    v, f = M.icosphere(0)
    pl = AU.placed(lambda s: s.mesh(v, f, mat=s.lambertian(s.solid(0.5, 0.5, 0.5))), [chain], 20)
    A, b, b1, (t0, t1), _ = pl.comp[0]
    seen = set()
    for T in V.TIMES:
        bT = V.off_at(b.astype(F32), b1.astype(F32), t0, t1, T)
        want = (v[f] @ A.T + bT.astype(np.float64)).astype(F32)
        got = M.flat_arrays(pl.scene.flat(time=T))[0][:, :9].reshape(-1, 3, 3)
        assert np.abs(got.astype(np.float64) - want) .max() <= np.spacing(np.abs(want)).max()
        seen.add(got.tobytes())
    assert len(seen) == len(V.TIMES)
    assert V.flats_equal(pl.scene.flat(), pl.scene.flat(time=0.0)) is None


# ---- 3. the checker against float64 ground truth -----------------------------------------
TRUTH = [nw.affine(axis=(1, 2, -1), angle=64.0, translate=(0.5, 0.25, -1.0)),
         nw.affine(scale=(2.0, 0.5, 1.0), translate=(-0.3, 0.4, 0.2)),
         AU.shear(0.5, translate=(1.0, -0.5, 0.3)),
         nw.affine(scale=(2.0, 0.5, 1.0), axis=(1, 1, 0), angle=40.0, translate=(0.2, 0.1, 0.0)) ]


@pytest.mark.parametrize("k", range(len(TRUTH)))
def test_checker_equals_double_precision_ground_truth(k):
    """The pattern, filters and tolerances of test_reference_equals_double_
    precision_ground_truth and test_reference_record_equals_double_precision:
    the few-ulp error those were set for grows by at most the condition number
    (<= 8 here) and stays an order of magnitude inside 1e-4."""
    m = TRUTH[k]
    assert np.linalg.cond(m[:, :3]) <= 8
    v, f = M.icosphere(2)
    pl = AU.placed(lambda s: s.mesh(v, f, mat=s.lambertian(s.solid(0.5, 0.5, 0.5))), [[("transform", m)]], 320)
    world = AU.world_triangles(pl, 0)
    g = np.random.default_rng(11 + k)
    n = 40_000
    centre = m[:, :3] @ np.array(M.CENTRE) + m[:, 3]
    o = centre + (g.random((n, 3)) - 0.5) * 14.0
    aim = centre + (g.normal(size=(n, 3)) * 0.6) @ m[:, :3].T
    rays = np.zeros((n, 7), F32)
    rays[:, :6] = np.column_stack([o, aim - o])
    ti, tt, cosv, edge = M.moller_trumbore(world, rays[:, :6])
    ri, rt, rp, rj = AU.affine_closest(pl, rays)
    hit = ti >= 0
    keep = hit & (cosv >= 0.1) & (edge >= 1e-4) & (np.abs(tt - 0.001) > 1e-5)
    print(f"matrix {k}: hit {hit.mean():.3f}, kept {keep.sum() / hit.sum():.3f} of them")
    assert hit.mean() > 0.5 and keep.sum() >= 0.5 * hit.sum()
    assert np.array_equal(ri[keep], ti[keep])
    rel = np.abs(rt[keep].astype(np.float64) - tt[keep]) / tt[keep]
    assert rel.max() <= 1e-4, rel.max()
    assert len(np.unique(ri[keep])) > 250
    rec, mat, side = AU.affine_records(pl, rays, np.where(keep, rp, -1), rj, rt)
    o64, d64 = rays[keep, :3].astype(np.float64), rays[keep, 3:6].astype(np.float64)
    p64 = o64 + tt[keep][:, None] * d64
    tri = world[ti[keep]]
    nn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nn /= np.linalg.norm(nn, axis=1)[:, None]
    assert np.abs(rec[keep, :3] - p64).max() < 1e-4 and np.abs(rec[keep, 3:6] - nn).max() < 1e-5
    assert (side[keep] == SU.SIDE_NONE).all() and (rec[keep, 6:8] == 0).all()


# ---- 4. the closed form ------------------------------------------------------------------
@pytest.mark.parametrize("m", [AU.shear(0.5, (1.5, 0.8, 1.0), (0.4, -0.2, 0.1)), nw.affine(scale=(1.0, 2.0, 0.7), axis=(1, 1, 1), angle=35.0)])
def test_smooth_normal_on_an_ellipsoid(m):
    """An icosphere of the unit sphere with the sphere's normals under (A, b) is
    an ellipsoid: the interpolated normal at local x is x exactly in real
    arithmetic, so the record's normal at p is normalize(A^-T A^-1 (p - b)) —
    which the matrix itself (A A^-1 (p - b), or A x) would not give."""
    v, f = M.icosphere(2, radius=1.0, centre=(0.0, 0.0, 0.0))
    pl = AU.placed(lambda s: s.mesh(v, f, normals=v, smooth=True, mat=s.lambertian(s.solid(0.5, 0.5, 0.5))), [[("transform", m)]], 320)
    A, b = m[:, :3], m[:, 3]
    g = np.random.default_rng(3)
    n = 20_000
    o = b + (g.random((n, 3)) - 0.5) * 8.0
    rays = np.zeros((n, 7), F32)
    rays[:, :6] = np.column_stack([o, b + (g.normal(size=(n, 3)) * 0.5) @ A.T - o])
    ri, rt, rp, rj = AU.affine_closest(pl, rays)
    rec, mat, side = AU.affine_records(pl, rays, rp, rj, rt)
    hit = ri >= 0
    took = hit & (side == SU.SIDE_SMOOTH)
    assert hit.mean() > 0.2 and took.sum() > 0.9 * hit.sum()
    Ai = np.linalg.inv(A)
    x = (rec[took, :3].astype(np.float64) - b) @ Ai.T  # A^-1 (p - b)
    want = x @ Ai  # rows (A^-T x)^T
    want /= np.linalg.norm(want, axis=1)[:, None]
    assert np.abs(rec[took, 3:6] - want).max() <= 1e-5, np.abs(rec[took, 3:6] - want).max()
    wrong = x @ A.T
    wrong /= np.linalg.norm(wrong, axis=1)[:, None]
    assert np.abs(rec[took, 3:6] - wrong).max() > 0.1  # the two differ, visibly


# ---- 5. watertightness ---------------------------------------------------------------------
def test_checker_is_watertight_under_a_sheared_placement():
    v, f = M.icosphere(2)
    m = AU.shear(0.5, (2.0, 0.5, 1.3), (0.7, -0.4, 0.2))
    pl = AU.placed(lambda s: s.mesh(v, f, mat=s.lambertian(s.solid(0.5, 0.5, 0.5))), [[("transform", m)]], 320)
    rays = AU.watertight_rays(m, v, f)
    ri, rt, _, _ = AU.affine_closest(pl, rays)
    assert len(rays) > 150_000 and (ri >= 0).all(), np.nonzero(ri < 0)[0][:10]
    assert len(np.unique(ri)) == 320


# ---- 6. the sanitizer program --------------------------------------------------------------
def _sanitizer_runtime_present(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    p = subprocess.run([CLANG, *SAN, "-o", str(tmp_path / "probe"), str(src)], capture_output=True, timeout=300)
    return p.returncode == 0


def test_affine_build_under_asan_ubsan(tmp_path):
    """A stand-alone program (tests/native/nw_affine_sanitize.cpp, its own main;
    nothing is preloaded) with the scene builder compiled under
    -fsanitize=address,undefined: the scenes of these tests through
    build_device_scene and the flat view, every affine placement's box checked
    against its mesh in double at 33 times in [0, 1], every bottom-level box
    against its triangles, the scenes destroyed (leaks are errors)."""
    if not os.path.exists(CLANG) or not _sanitizer_runtime_present(tmp_path):
        pytest.skip("the compiler lacks the sanitizer runtime")
    exe = tmp_path / "nw_affine_sanitize"
    cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", *SAN, "-o", str(exe),
           os.path.join(REPO, "tests", "native", "nw_affine_sanitize.cpp"), os.path.join(CSRC, "rtmi_nw_scene.cpp"),
           os.path.join(CSRC, "rtmi_host.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    path = tmp_path / "cube.obj"
    path.write_text(M.cube_obj("a//n", quads=True))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               LSAN_OPTIONS="suppressions=" + os.path.join(REPO, "tests", "native", "lsan.supp"),
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "all checks passed" in p.stdout


# ---- 7. the CLI ------------------------------------------------------------------------------
def test_cli_rejects_obj_tumble_without_obj():
    exe = os.path.join(os.path.dirname(nw.__file__), "bin", "rtmi_nw_render")
    p = subprocess.run([exe, "--scene", "2", "--obj-tumble"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "--obj-tumble" in p.stderr


def test_obj_stage_tumbled(tmp_path):
    path = tmp_path / "cube.obj"
    path.write_text(M.cube_obj("a//n", quads=True, scale=2.0, offset=(-1.0, 0.0, -1.0)))  # the stage's box: staged as it is
    still, cam0, _ = nw.obj_stage(path, copies=2)
    s, cam, n = nw.obj_stage(path, copies=2, tumble=True)
    assert n == 12 and bytes(cam) == bytes(cam0) and s.affine_stats() == (4, 0) and s.motion_stats() == (0, 4)
    assert still.affine_stats() == (0, 4) and s.instancing_stats()["pool_triangles"] == 12
    obj = M.flat_arrays(s.flat())[0]
    tri = obj[obj[:, 12].view(np.int32) == 7][:, :9].reshape(4, 12, 3, 3).astype(np.float64)
    for q in range(4):
        i, k = divmod(q, 2)
        lo, hi = tri[q].reshape(-1, 3).min(axis=0), tri[q].reshape(-1, 3).max(axis=0)
        assert abs(lo[1]) < 1e-6  # the lowest corner of the cube (the stage box itself) stands on the ground
        edge = np.linalg.norm(tri[q][:, 1] - tri[q][:, 0], axis=1).min()
        assert abs(edge - 2.0 * (0.75 + 0.25 * np.sin(2.9 * q))) < 1e-5  # the uniform scale
        centre = (3.0 * (i - 0.5) + 0.4 * np.sin(1.7 * q), 3.0 * (k - 0.5) + 0.4 * np.cos(2.3 * q))
        assert abs((lo[0] + hi[0]) / 2 - centre[0]) < 1.5 and abs((lo[2] + hi[2]) / 2 - centre[1]) < 1.5
    both, _, _ = nw.obj_stage(path, copies=2, tumble=True, move=(0, 0.4, 0))
    assert both.affine_stats() == (4, 0) and both.motion_stats() == (4, 0)
    # at rest it is the static field (a moving placement bakes the float offset, a static one the double: an ulp)
    is_tri = obj[:, 12].view(np.int32) == 7

    def verts(scene, T):  # (the nine vertex floats of the triangle rows)
        return M.flat_arrays(scene.flat(time=T))[0][is_tri][:, :9]

    assert np.abs(verts(both, 0.0) - verts(s, 0.0)).max() < 1e-6
    up = verts(both, 0.5) - verts(s, 0.0)
    assert np.abs(up[:, [1, 4, 7]] - 0.2).max() < 1e-6 and np.abs(up[:, [0, 2, 3, 5, 6, 8]]).max() < 1e-6
    one, _, _ = nw.obj_stage(path, copies=1, tumble=True)
    assert one.affine_stats() == (1, 0)
    assert _code(lambda: nw.obj_stage(path, copies=0, tumble=True)) == EINVAL
    assert _code(lambda: nw.obj_stage(path, copies=257, tumble=True)) == EINVAL
