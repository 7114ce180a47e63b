"""Shared meshes in the Next-Week renderer (Scene.shared, rt_nw_shared), on the
CPU: the flat view of a scene with placements is the flattened copies' byte for
byte, the counts of the two-level build, what cannot be shared, and the host
build under ASan + UBSan (tests/native/nw_instance_sanitize.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import nw_instance_util as U
import nw_mesh_util as M
from a_dive_into_ray_tracing_amd import _abi, nextweek as nw

REPO = M.REPO
CSRC = os.path.join(REPO, "a_dive_into_ray_tracing_amd", "csrc")
CLANG = "/opt/rocm/llvm/bin/clang++"
EINVAL, EUNSUPPORTED = -1, -4  # include/rtmi.h
SAN = ["-fsanitize=address", "-fsanitize=undefined", "-fno-sanitize-recover=all"]  # the Makefile's SAN


def test_flat_view_is_the_expansion():
    a, b = U.five_placements(True), U.five_placements(False)
    fa, fb = a.flat(), b.flat()
    assert fa["n_obj"] == fb["n_obj"] == 5 * 320 + len(U.SPHERES)
    assert sorted(fa) == sorted(fb)
    for key in fb:
        x, y = np.asarray(fa[key]), np.asarray(fb[key])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), key
    _, inst = M.flat_arrays(fa)
    assert len(inst) == 3  # translate, rotate_y, both: the repeated placement shares its Inst
    aa, ab = a.flat_attr(), b.flat_attr()
    for key in ab:
        assert aa[key].tobytes() == ab[key].tobytes(), key


def test_flat_view_with_attributes_is_the_expansion():
    import nw_smooth_util as SU

    def build(shared):
        s = nw.Scene()
        v, f = M.icosphere(1)
        uv = np.random.default_rng(3).random((len(v), 2))
        mesh = s.mesh(v, f, normals=SU.sphere_normals(v), uvs=uv, smooth=True, mat=s.lambertian(s.solid(0.5, 0.5, 0.5)))
        h = s.shared(mesh) if shared else mesh
        s.add(s.translate(h, (1, 2, 3)))
        s.add(s.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), s.lambertian(s.solid(0.1, 0.2, 0.3))))
        s.add(s.rotate_y(h, 40))
        return s

    a, b = build(True), build(False)
    for x, y in ((a.flat(), b.flat()), (a.flat_attr(), b.flat_attr())):
        for key in y:
            assert np.asarray(x[key]).tobytes() == np.asarray(y[key]).tobytes(), key
    assert (b.flat_attr()["attr_of_obj"] >= 0).sum() == 160
    assert a.instancing_stats()["pool_triangles"] == 80


def test_instancing_stats():
    st = U.five_placements(True).instancing_stats()
    assert (st["meshes"], st["placements"], st["pool_triangles"]) == (1, 5, 320)
    assert st["top_leaves"] == 5 + len(U.SPHERES)
    assert 320 // 4 <= st["bottom_nodes"] < 2 * 320 and st["top_leaves"] <= st["top_nodes"] < 2 * st["top_leaves"]
    plain = U.five_placements(False).instancing_stats()
    assert (plain["meshes"], plain["placements"], plain["pool_triangles"], plain["bottom_nodes"]) == (0, 0, 0, 0)
    assert plain["top_leaves"] == 5 * 320 + len(U.SPHERES)
    # a collinear triangle is counted by the flat view and stays out of the pool
    c = U.five_placements(True, collinear=True)
    assert c.flat()["n_obj"] == 5 * 321 + len(U.SPHERES)
    assert c.instancing_stats()["pool_triangles"] == 320 and c.instancing_stats()["top_leaves"] == 5 + len(U.SPHERES)
    assert c.flat()["obj"].tobytes() == U.five_placements(False, collinear=True).flat()["obj"].tobytes()


def _code(fn):
    with pytest.raises(_abi.RTError) as e:
        fn()
    return e.value.code


def test_what_cannot_be_shared():
    s = nw.Scene()
    mat = s.lambertian(s.solid(0.5, 0.5, 0.5))
    v, f = M.icosphere(0)
    mesh = s.mesh(v, f, mat=mat)
    h = s.shared(mesh)
    assert h >= 0 and s.shared(s.group([mesh, s.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), mat)])) >= 0
    assert _code(lambda: s.shared(s.sphere((0, 0, 0), 1, mat))) == EUNSUPPORTED
    assert _code(lambda: s.shared(s.translate(mesh, (1, 0, 0)))) == EUNSUPPORTED
    assert _code(lambda: s.shared(s.group([mesh, s.rotate_y(mesh, 5)]))) == EUNSUPPORTED
    assert _code(lambda: s.shared(h)) == EUNSUPPORTED
    assert _code(lambda: s.shared(s.group([]))) == EINVAL
    assert _code(lambda: s.shared(-1)) == EINVAL
    assert _code(lambda: s.shared(10 ** 6)) == EINVAL
    assert _code(lambda: s.constant_medium(h, 0.1, s.solid(1, 1, 1))) == EUNSUPPORTED
    assert _code(lambda: s.constant_medium(s.translate(h, (0, 1, 0)), 0.1, s.solid(1, 1, 1))) == EUNSUPPORTED
    # a shared handle inside a group is a placement like any other
    s.add(s.translate(s.group([h, s.sphere((5, 0, 0), 1, mat)]), (0, 0, 2)))
    s.add(h)
    st = s.instancing_stats()
    assert (st["meshes"], st["placements"], st["pool_triangles"], st["top_leaves"]) == (1, 2, 20, 3)


def test_a_scene_with_a_placement_has_no_grid():
    assert U.five_placements(True).grid_stats()["dims"] == (0, 0, 0)
    assert U.five_placements(False).grid_stats()["dims"] != (0, 0, 0)


def test_obj_stage_copies(tmp_path):
    path = tmp_path / "cube.obj"
    path.write_text(M.cube_obj("a//n", quads=True))
    one, cam1, n = nw.obj_stage(path, copies=1)
    plain, cam0, _ = nw.obj_stage(path)
    assert n == 12 and one.flat()["obj"].tobytes() == plain.flat()["obj"].tobytes() and bytes(cam1) == bytes(cam0)
    assert one.instancing_stats()["placements"] == 0
    s, cam, n = nw.obj_stage(path, copies=3)
    st = s.instancing_stats()
    assert n == 12 and (st["meshes"], st["placements"], st["pool_triangles"], st["top_leaves"]) == (1, 9, 12, 11)
    _, inst = M.flat_arrays(s.flat())
    assert s.flat()["n_obj"] == 9 * 12 + 2 and len(inst) == 9  # every copy its own rotation and translation
    assert len(np.unique(inst[:, :5], axis=0)) == 9
    assert _code(lambda: nw.obj_stage(path, copies=0)) == EINVAL
    assert _code(lambda: nw.obj_stage(path, copies=257)) == EINVAL


def _sanitizer_runtime_present(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    p = subprocess.run([CLANG, *SAN, "-o", str(tmp_path / "probe"), str(src)], capture_output=True, timeout=300)
    return p.returncode == 0


def test_two_level_build_under_asan_ubsan(tmp_path):
    """A stand-alone program (tests/native/nw_instance_sanitize.cpp, its own
    main; nothing is preloaded) with the scene builder compiled under
    -fsanitize=address,undefined: the five-placement scene and icosphere(4) x 3
    through build_device_scene, every bottom-level box, link and placement box
    checked, the scenes destroyed (leaks are errors)."""
    if not os.path.exists(CLANG) or not _sanitizer_runtime_present(tmp_path):
        pytest.skip("the compiler lacks the sanitizer runtime")
    exe = tmp_path / "nw_instance_sanitize"
    cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", *SAN, "-o", str(exe),
           os.path.join(REPO, "tests", "native", "nw_instance_sanitize.cpp"), os.path.join(CSRC, "rtmi_nw_scene.cpp"),
           os.path.join(CSRC, "rtmi_host.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               LSAN_OPTIONS="suppressions=" + os.path.join(REPO, "tests", "native", "lsan.supp"),
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "all checks passed" in p.stdout
