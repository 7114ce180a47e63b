"""Moving placements of shared meshes (Scene.move, rt_nw_move) on the CPU: the
flat view at an instant T (Scene.flat(time=T), rt_nw_scene_flat_at) holds
off(T) as numpy float32 evaluates the specification, and equals a hand-built
frozen scene byte for byte; scenes without a move node are what they were;
what cannot move; the CLI's argument check; and the host build under ASan +
UBSan (tests/native/nw_motion_sanitize.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import nw_instance_util as U
import nw_mesh_util as M
import nw_motion_util as V
from a_dive_into_ray_tracing_amd import _abi, nextweek as nw

REPO = M.REPO
CSRC = os.path.join(REPO, "a_dive_into_ray_tracing_amd", "csrc")
CLANG = "/opt/rocm/llvm/bin/clang++"
EINVAL, EUNSUPPORTED = -1, -4  # include/rtmi.h
SAN = ["-fsanitize=address", "-fsanitize=undefined", "-fno-sanitize-recover=all"]  # the Makefile's SAN


@pytest.fixture(scope="module")
def ends():
    return V.m_ends()


# ---- 1. the offsets are the formula's, everything else the static build's --------
@pytest.mark.parametrize("T", V.TIMES)
def test_flat_at_time_holds_the_formula(T, ends):
    moving = V.scene_m("moving")
    static = V.scene_m("end0").flat()
    got = moving.flat(time=T)
    assert sorted(got) == sorted(static)
    for key in static:
        if key != "inst":
            assert np.asarray(got[key]).tobytes() == np.asarray(static[key]).tobytes(), key
    gi, si = M.flat_arrays(got)[1], M.flat_arrays(static)[1]
    assert gi.shape == si.shape == (3, 8)
    want = si.copy()
    want[1, 2:5] = V.off_at(*ends[0], 0.0, 1.0, T)
    want[2, 2:5] = V.off_at(*ends[1], V.C_T0, V.C_T1, T)
    assert gi.tobytes() == want.tobytes(), (T, gi, want)
    assert (gi[:, 5].view(np.int32) & 2).all()  # the translation flag
    # the two ends are not where the third placement stands: it extrapolates outside [0.25, 0.75]
    if T in (0.0, 1.0):
        assert not np.array_equal(gi[2, 2:5], ends[1][int(T)])
    assert moving.motion_stats() == (2, 1)


def test_flat_without_time_is_time_zero(ends):
    s = V.scene_m("moving")
    assert V.flats_equal(s.flat(), s.flat(time=0.0)) is None
    assert V.flats_equal(s.flat(time=0.5), s.flat(time=0.0)) == "inst"
    # offset0 == offset1 is legal and stands still
    a = nw.Scene()
    v, f = M.icosphere(0)
    h = a.shared(a.mesh(v, f, mat=a.lambertian(a.solid(0.5, 0.5, 0.5))))
    a.add(a.move(h, (1, 2, 3), (1, 2, 3), 0.2, 0.9))
    assert V.flats_equal(a.flat(time=0.0), a.flat(time=0.77)) is None and a.motion_stats() == (1, 0)


# ---- 2. the frozen scene ------------------------------------------------------------
@pytest.mark.parametrize("T", V.TIMES)
def test_flat_at_time_is_the_frozen_scene(T, ends):
    moving, frozen = V.scene_m("moving"), V.scene_m("frozen", T, ends[1])
    assert V.flats_equal(moving.flat(time=T), frozen.flat()) is None
    assert V.flats_equal(moving.flat_attr(), frozen.flat_attr()) is None
    assert frozen.motion_stats() == (0, 3)
    # the literal tree — rotate_y(translate(h, x), 20) — differs from it in that one row at most, and the
    # row expected there is the formula's (checked above): every other byte is the same
    lit = V.scene_m("end0").flat()
    assert [k for k in lit if np.asarray(lit[k]).tobytes() != np.asarray(frozen.flat()[k]).tobytes()] in ([], ["inst"])


@pytest.mark.parametrize("build", [V.scene_s, V.scene_f, V.scene_x, V.scene_l])
def test_other_scenes_freeze_too(build):
    for T in (0.0, float(np.float32(1) / np.float32(3)), 1.0):
        moving, frozen = build("moving"), build("frozen", T)
        assert V.flats_equal(moving.flat(time=T), frozen.flat()) is None, T
        assert V.flats_equal(moving.flat_attr(), frozen.flat_attr()) is None, T
        assert moving.motion_stats()[0] >= 1 and frozen.motion_stats()[0] == 0
        assert moving.instancing_stats()["placements"] == sum(frozen.motion_stats())


# ---- 3. scenes without a move node ---------------------------------------------------
def test_scenes_without_a_move_are_unchanged():
    for build, n in ((lambda: U.five_placements(True), 5), (lambda: U.five_placements(False), 0), (lambda: U.mixed_placements(True), 3)):
        s = build()
        f0, a0 = s.flat(), s.flat_attr()
        assert V.flats_equal(s.flat(time=0.7), f0) is None and V.flats_equal(s.flat_attr(), a0) is None
        assert V.flats_equal(s.flat(), f0) is None
        assert s.motion_stats() == (0, n)
    # ... and the shared build's flat view is still the flattened copies' (today's bytes)
    assert V.flats_equal(U.five_placements(True).flat(time=0.7), U.five_placements(False).flat()) is None
    s, cam = nw.preset("cornell_smoke")
    assert V.flats_equal(s.flat(time=0.3), s.flat()) is None and s.motion_stats() == (0, 0)


# ---- 4. what cannot move ----------------------------------------------------------------
def _code(fn):
    with pytest.raises(_abi.RTError) as e:
        fn()
    return e.value.code


def test_what_cannot_move():
    s = nw.Scene()
    mat = s.lambertian(s.solid(0.5, 0.5, 0.5))
    v, f = M.icosphere(0)
    mesh = s.mesh(v, f, mat=mat)
    h = s.shared(mesh)
    a, b = (0, 0, 0), (1, 0, 0)
    assert s.move(h, a, b) >= 0 and s.move(h, a, a) >= 0 and s.move(s.translate(s.rotate_y(h, 5), b), a, b, 0.25, 0.75) >= 0
    assert s.move(h, a, b, 1.0, 0.0) >= 0  # time1 < time0 is a line like any other
    assert _code(lambda: s.move(h, a, b, 0.5, 0.5)) == EINVAL
    assert _code(lambda: s.move(h, a, b, float("nan"), 1.0)) == EINVAL
    assert _code(lambda: s.move(h, a, b, 0.0, float("inf"))) == EINVAL
    assert _code(lambda: s.move(h, (0, float("nan"), 0), b)) == EINVAL
    assert _code(lambda: s.move(h, a, (1e39, 0, 0))) == EINVAL  # not finite as a float
    assert _code(lambda: s.move(-1, a, b)) == EINVAL and _code(lambda: s.move(10 ** 6, a, b)) == EINVAL
    sph = s.sphere((0, 0, 0), 1, mat)
    assert _code(lambda: s.move(sph, a, b)) == EUNSUPPORTED  # a moving primitive
    assert _code(lambda: s.move(mesh, a, b)) == EUNSUPPORTED  # a flattened mesh
    assert _code(lambda: s.move(s.translate(mesh, b), a, b)) == EUNSUPPORTED
    assert _code(lambda: s.move(s.group([h]), a, b)) == EUNSUPPORTED  # a group
    assert _code(lambda: s.move(s.group([h, h]), a, b)) == EUNSUPPORTED
    assert _code(lambda: s.move(s.constant_medium(sph, 0.1, s.solid(1, 1, 1)), a, b)) == EUNSUPPORTED
    mv = s.move(h, a, b)
    assert _code(lambda: s.move(mv, a, b)) == EUNSUPPORTED  # a move above a move
    assert _code(lambda: s.move(s.rotate_y(s.translate(mv, b), 3), a, b)) == EUNSUPPORTED
    assert _code(lambda: s.shared(mv)) == EUNSUPPORTED
    assert _code(lambda: s.constant_medium(mv, 0.1, s.solid(1, 1, 1))) == EUNSUPPORTED
    assert _code(lambda: s.constant_medium(s.translate(mv, b), 0.1, s.solid(1, 1, 1))) == EUNSUPPORTED
    # a move handle goes where a translate handle goes
    s.add(s.translate(s.group([mv, sph]), (0, 0, 2)))
    s.add(s.rotate_y(mv, 10))
    s.add(h)
    assert s.motion_stats() == (2, 1) and s.instancing_stats()["placements"] == 3
    assert _code(lambda: s.flat(time=float("nan"))) == EINVAL


# ---- 5. the CLI ----------------------------------------------------------------------------
def test_cli_rejects_obj_move_without_obj(tmp_path):
    exe = os.path.join(os.path.dirname(nw.__file__), "bin", "rtmi_nw_render")
    p = subprocess.run([exe, "--scene", "2", "--obj-move", "0,0.4,0"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "--obj-move" in p.stderr
    path = tmp_path / "cube.obj"
    path.write_text(M.cube_obj("a//n", quads=True))
    for bad in (["--obj-move", "0,0.4"], ["--obj-move", "0,x,1"], ["--obj-move", "0,0.4,0,1"], ["--shutter", "0.5"],
                ["--shutter", "0.6,0.5"], ["--shutter", "0,1.5"]):
        p = subprocess.run([exe, "--obj", str(path), *bad], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and bad[0] in p.stderr, (bad, p.returncode, p.stderr)


def test_obj_stage_moving(tmp_path):
    path = tmp_path / "cube.obj"
    path.write_text(M.cube_obj("a//n", quads=True))
    still, cam0, _ = nw.obj_stage(path, copies=2)
    s, cam, n = nw.obj_stage(path, copies=2, move=(0, 0.4, 0))
    assert n == 12 and bytes(cam) == bytes(cam0) and s.motion_stats() == (4, 0) and still.motion_stats() == (0, 4)
    assert V.flats_equal(s.flat(time=0.0), still.flat()) is None
    gi, si = M.flat_arrays(s.flat(time=0.5))[1], M.flat_arrays(still.flat())[1]
    want = si.copy()
    want[:, 3] = np.float32(0.5) * np.float32(0.4)
    assert gi.tobytes() == want.tobytes()
    one, _, _ = nw.obj_stage(path, copies=1, move=(0.25, 0, 0))
    assert one.motion_stats() == (1, 0) and one.instancing_stats()["pool_triangles"] == 12
    assert _code(lambda: nw.obj_stage(path, copies=0, move=(0, 1, 0))) == EINVAL
    assert _code(lambda: nw.obj_stage(path, copies=2, move=(0, float("inf"), 0))) == EINVAL


# ---- 6. the sanitizer program ---------------------------------------------------------------
def _sanitizer_runtime_present(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    p = subprocess.run([CLANG, *SAN, "-o", str(tmp_path / "probe"), str(src)], capture_output=True, timeout=300)
    return p.returncode == 0


def test_moving_build_under_asan_ubsan(tmp_path):
    """A stand-alone program (tests/native/nw_motion_sanitize.cpp, its own main;
    nothing is preloaded) with the scene builder compiled under
    -fsanitize=address,undefined: the scenes of these tests through
    build_device_scene and the flat view at several times, every moving
    placement's box checked against its mesh at 33 times in [0, 1], the scenes
    destroyed (leaks are errors)."""
    if not os.path.exists(CLANG) or not _sanitizer_runtime_present(tmp_path):
        pytest.skip("the compiler lacks the sanitizer runtime")
    exe = tmp_path / "nw_motion_sanitize"
    cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", *SAN, "-o", str(exe),
           os.path.join(REPO, "tests", "native", "nw_motion_sanitize.cpp"), os.path.join(CSRC, "rtmi_nw_scene.cpp"),
           os.path.join(CSRC, "rtmi_host.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               LSAN_OPTIONS="suppressions=" + os.path.join(REPO, "tests", "native", "lsan.supp"),
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "all checks passed" in p.stdout
