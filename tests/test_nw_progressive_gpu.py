"""Progressive passes of the Next-Week renderer on the GPU (rt_nw_accum_* /
rt_nw_render_pass, DESIGN.md §9 "Progressive passes").

  * any split of [0, S) into passes, in any order, under any accelerator and
    kernel shape and for every mesh family, resolves to the sums of one
    rt_nw_render of S samples bit for bit (and to the oracle's where it can
    render the scene), and the passes' world.hit counts add up;
  * passes above one work item's 65 535 samples, on row strips and torch
    streams, around plain renders and resolves, through export / import and
    through checkpoint files (refused when made for another render);
  * the argument checks, and the CLI's --pass-spp / --checkpoint / --time-limit.
"""
import copy
import os
import random
import subprocess

import numpy as np
import pytest

import a_dive_into_ray_tracing_amd.nextweek as nw
import nw_affine_util as AU
import nw_mesh_util as M
import nw_motion_util as V
import oracle_py as O
from a_dive_into_ray_tracing_amd._abi import RTError

pytestmark = pytest.mark.gpu
GOLD = O.GOLDEN
SEED = 1984
W, H, S = 29, 23, 24  # partial 8 x 8 tiles on both axes
SPLITS = [[24], [1, 23], [7, 5, 12], [3] * 8]
CLI = os.path.join(os.path.dirname(nw.__file__), "bin", "rtmi_nw_render")
RT_EINVAL = -1


def ranges(split):
    out, s = [], 0
    for k in split:
        out.append((s, k))
        s += k
    return out


def run_passes(r, cam, w, h, rgs, depth=50, seed=SEED):
    """(resolved sums, summed world.hit counts) of the passes rgs = [(s_begin, s_count), ...]."""
    r.accum_reset(w, h)
    segs = 0
    for s0, k in rgs:
        r.render_pass(cam, w, h, s0, k, depth, seed)
        segs += r.last_segments()
    return r.resolve(), segs


@pytest.fixture(scope="module")
def earth():
    return nw.load_image(os.path.join(GOLD, "earthmap.jpeg"))


_REF = {}


def preset_ref(which, earth):
    """(scene, camera, oracle sums, oracle segments) of a preset at W x H x S: computed once."""
    if which not in _REF:
        s, cam = nw.preset(which, image=earth, aspect=W / H)
        want, segs = O.nw_render(s.flat(), cam, W, H, S, 50, SEED)
        want.setflags(write=False)
        _REF[which] = (s, cam, want, segs)
    return _REF[which]


# ---- splits equal the single render and the oracle ------------------------------------
@pytest.mark.parametrize("accel", ["bvh", "grid"])
@pytest.mark.parametrize("which", [1, 7, 8])
def test_splits_equal_single_render_and_oracle(which, accel, earth):
    s, cam, want, want_segs = preset_ref(which, earth)
    r = nw.NwRenderer(s)
    try:
        r.set_accel(accel)
        if r.accel_info()["accel"] != accel:  # (a scene without a grid renders "grid" with the BVH: covered by "bvh")
            assert accel == "grid" and which != 1
            return
        single = r.render(cam, W, H, S, 50, SEED)
        assert r.last_segments() == want_segs
        assert np.array_equal(single, want)
        if which == 1 and accel == "grid":
            assert r.last_kernel()["spheres_only"] == 1 and r.last_kernel()["persistent"] == 1
        shuffled = ranges([7, 5, 12])
        random.Random(3).shuffle(shuffled)
        assert shuffled != ranges([7, 5, 12])
        for rgs in [ranges(sp) for sp in SPLITS] + [shuffled]:
            got, segs = run_passes(r, cam, W, H, rgs)
            assert np.array_equal(got, single), rgs
            assert np.array_equal(got, want), rgs
            assert segs == want_segs, rgs
    finally:
        r.close()


# ---- mesh scenes ----------------------------------------------------------------------
def mesh_cam(t0=0.0, t1=1.0):
    return nw.camera((6, 2.5, 7), M.CENTRE, (0, 1, 0), 35, W / H, 0.0, 9.0, t0, t1)


def flat_mesh_scene():
    """Family 1: flat triangles (an icosphere) among spheres over a ground sphere; it has a uniform grid."""
    s = nw.Scene()
    grey = s.lambertian(s.solid(0.6, 0.5, 0.4))
    v, f = M.icosphere(2)
    s.add(s.mesh(v, f, mat=grey))
    s.add(s.sphere((2.5, -0.2, 0.9), 0.9, s.metal(s.solid(0.7, 0.6, 0.5), 0.0)))
    s.add(s.sphere((-1.9, -0.2, 0.9), 0.9, s.dielectric(1.5)))
    s.add(s.sphere((0, -1002, 0), 1000, s.lambertian(s.checker(s.solid(0.2, 0.3, 0.1), s.solid(0.9, 0.9, 0.9)))))
    s.set_background(0.7, 0.8, 1.0)
    return s


def family5_scene():
    """One shared mesh with a static, a moving and an affine placement (nw_affine_util's chains)."""
    return AU.scene_a(chains=[AU.A_CHAINS[0], AU.A_CHAINS[4], AU.A_CHAINS[1]]).scene


def family5_cam():
    return nw.camera((2.0, 4.5, 15.0), (0.4, 0.4, 1.4), (0, 1, 0), 40, W / H, 0.0, 10.0, 0.0, 1.0)


MESH_SCENES = {
    # name: (builder, camera, family, accelerator, the oracle renders its flat view bit for bit)
    "flat_grid": (flat_mesh_scene, mesh_cam, 1, "grid", True),
    "shared_static": (lambda: V.scene_m("end0"), mesh_cam, 3, "bvh", True),
    "shared_moving": (lambda: V.scene_m("moving"), mesh_cam, 4, "bvh", False),
    "shared_affine": (family5_scene, family5_cam, 5, "bvh", False),
}


@pytest.mark.parametrize("name", list(MESH_SCENES))
def test_mesh_families(name):
    build, cam_of, family, accel, oracle = MESH_SCENES[name]
    s, cam = build(), cam_of()
    r = nw.NwRenderer(s)
    try:
        r.set_accel(accel)
        assert r.scene_tri() == family and r.accel_info()["accel"] == accel
        single = r.render(cam, W, H, S, 50, SEED)
        single_segs = r.last_segments()
        assert np.isfinite(single).all() and len(np.unique(single.reshape(-1, 3), axis=0)) > 20
        for sp in SPLITS:
            got, segs = run_passes(r, cam, W, H, ranges(sp))
            assert np.array_equal(got, single), sp
            assert segs == single_segs, sp
        if oracle:
            want, want_segs = O.nw_render(s.flat(), cam, W, H, S, 50, SEED)
            assert np.array_equal(single, want) and single_segs == want_segs
    finally:
        r.close()


# ---- kernel shapes ----------------------------------------------------------------------
@pytest.mark.parametrize("env,key,value", [("RTMI_NW_PERSIST", "0", ("persistent", 0)), ("RTMI_NW_CHUNK", "4", ("chunk", 4))],
                         ids=["one_shot", "chunk4"])
@pytest.mark.parametrize("scene", ["preset7", "flat_grid", "shared_affine"])
def test_kernel_shapes(scene, env, key, value, earth, monkeypatch):
    """[7, 5, 12] with the one-shot kernels, and with 4 samples per work item: a pass of 7 is then two items, one partial."""
    if scene == "preset7":
        s, cam, _, _ = preset_ref(7, earth)
        accel = "bvh"
    else:
        build, cam_of, _, accel, _ = MESH_SCENES[scene]
        s, cam = build(), cam_of()
    r = nw.NwRenderer(s)  # (the default shape)
    try:
        r.set_accel(accel)
        single = r.render(cam, W, H, S, 50, SEED)
        single_segs = r.last_segments()
        assert r.last_kernel()["persistent"] == 1
    finally:
        r.close()
    monkeypatch.setenv(env, key)  # read when the context is created
    r = nw.NwRenderer(s)
    try:
        r.set_accel(accel)
        r.accum_reset(W, H)
        segs = 0
        for s0, k in ranges([7, 5, 12]):
            r.render_pass(cam, W, H, s0, k, 50, SEED)
            assert r.last_kernel()[value[0]] == value[1], r.last_kernel()
            segs += r.last_segments()
        assert np.array_equal(r.resolve(), single)
        assert segs == single_segs
    finally:
        r.close()


# ---- past one item's limit ---------------------------------------------------------------
def test_passes_above_one_items_samples():
    """[0, 70 000) needs two items per tile (at most 65 535 samples each); [70 000, 70 003) starts above 65 535."""
    w = h = 8
    s, cam = nw.preset(2, aspect=1.0)
    r = nw.NwRenderer(s)
    try:
        want = r.render(cam, w, h, 70_003, 50, SEED)
        got, _ = run_passes(r, cam, w, h, [(0, 70_000), (70_000, 3)])
        assert np.array_equal(got, want)
    finally:
        r.close()


# ---- strips --------------------------------------------------------------------------------
def test_strip_passes_on_a_torch_stream(earth):
    import torch

    w, h = 24, 40
    row0, step, nrows = 1, 3, 14  # rows 1, 4, ..., 37, then one past H: zero
    s, cam = nw.preset(8, image=earth, aspect=1.0)
    r = nw.NwRenderer(s)
    try:
        st = torch.cuda.Stream()
        want = torch.full((nrows, w, 3), -1.0, dtype=torch.float32, device="cuda")
        r.render_rows(cam, w, h, S, 50, SEED, row0, step, nrows, want.data_ptr(), st.cuda_stream)
        st.synchronize()
        r.accum_reset(w, nrows)
        for s0, k in ranges([7, 5, 12]):
            r.render_pass(cam, w, h, s0, k, 50, SEED, row0, step, nrows, stream=st.cuda_stream)
        got = torch.full((nrows, w, 3), -1.0, dtype=torch.float32, device="cuda")
        r.resolve(dev_ptr=got.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        got, want = got.cpu().numpy(), want.cpu().numpy()
        assert np.array_equal(got, want)
        assert (got[13] == 0).all() and (got[:13] > 0).any()
        assert np.array_equal(r.resolve(), want)  # on the context's stream: waits for the passes
    finally:
        r.close()


# ---- isolation ------------------------------------------------------------------------------
def test_renders_and_resolves_between_passes_change_nothing(earth):
    s, cam, want, _ = preset_ref(7, earth)
    cam2 = nw.camera((278, 278, -800), (278, 278, 0), (0, 1, 0), 40, 40 / 16, 0.0, 10.0)
    r = nw.NwRenderer(s)
    try:
        r.accum_reset(W, H)
        r.render_pass(cam, W, H, 0, 7)
        other = r.render(cam2, 40, 16, 70, 50, SEED + 1)  # chunked: uses the context's own accumulator and scratch
        assert np.isfinite(other).all()
        mid = r.resolve()
        r.render_pass(cam, W, H, 7, 5)
        assert np.array_equal(r.resolve(), r.resolve())
        r.render_pass(cam, W, H, 12, 12)
        assert np.array_equal(r.resolve(), want)
        seven, _ = run_passes(r, cam, W, H, [(0, 7)])
        assert np.array_equal(mid, seven)
    finally:
        r.close()


# ---- export and import ---------------------------------------------------------------------
def test_export_import(earth):
    s, cam, want, _ = preset_ref(8, earth)
    r = nw.NwRenderer(s)
    try:
        r.accum_reset(W, H)
        r.render_pass(cam, W, H, 0, 10)
        raw10, done = r.accum_export()
        assert done == 10 and raw10.dtype == np.int64 and raw10.shape == (H, W, 3)
        r.accum_reset(W, H)
        assert not r.accum_export()[0].any()
        r.accum_import(raw10, 10)
        r.render_pass(cam, W, H, 10, 14)
        assert np.array_equal(r.resolve(), want)
        raw24, done = r.accum_export()
        assert done == 24
        r.accum_reset(W, H)
        r.render_pass(cam, W, H, 10, 14)
        raw_tail, done = r.accum_export()
        assert done == 14 and np.array_equal(raw_tail, raw24 - raw10)
    finally:
        r.close()


# ---- checkpoints ------------------------------------------------------------------------------
class Stop(Exception):
    pass


def test_checkpoint_resume_under_the_other_accelerator(earth, tmp_path):
    s, cam, want, _ = preset_ref(1, earth)
    ck = str(tmp_path / "run.ckpt")
    seen = []

    def stop_after_two(done):
        seen.append(done)
        if len(seen) == 2:
            raise Stop

    r = nw.NwRenderer(s)
    try:
        r.set_accel("grid")
        assert r.accel_info()["accel"] == "grid"
        with pytest.raises(Stop):
            r.progressive(cam, W, H, S, 6, 50, SEED, checkpoint=ck, on_pass=stop_after_two)
    finally:
        r.close()
    assert seen == [6, 12] and os.path.exists(ck) and not os.path.exists(ck + ".tmp")
    info = nw.accum_info(ck)
    assert (info["W"], info["H"], info["nrows"], info["spp_done"], info["max_depth"], info["seed"]) == (W, H, H, 12, 50, SEED)
    assert info["scene_hash"] == s.hash()
    s2, cam_b = nw.preset(1, image=earth, aspect=W / H)  # the same scene, built again
    fresh = nw.NwRenderer(s2)
    try:
        fresh.set_accel("bvh")
        shut = copy.copy(cam)
        shut.time1 = 0.5
        for kw in (dict(seed=SEED + 1), dict(max_depth=49), dict(cam=shut), dict(W=W + 1)):
            a = dict(cam=cam_b, W=W, H=H, spp=S, pass_spp=6, max_depth=50, seed=SEED, checkpoint=ck)
            a.update(kw)
            with pytest.raises(RTError, match="another render") as e:
                fresh.progressive(**a)
            assert e.value.code == RT_EINVAL
        resumed = []
        got = fresh.progressive(cam_b, W, H, S, 6, 50, SEED, checkpoint=ck, on_pass=resumed.append)
        assert resumed == [18, 24]
        assert np.array_equal(got, want)
        assert nw.accum_info(ck)["spp_done"] == 24
    finally:
        fresh.close()


def test_checkpoint_refuses_a_scene_with_another_move_offset(tmp_path):
    ck = str(tmp_path / "move.ckpt")
    cam = V.camera_l(16, 16)
    r = nw.NwRenderer(V.scene_l())
    try:
        r.progressive(cam, 16, 16, 4, 2, 50, SEED, checkpoint=ck)
    finally:
        r.close()
    l1 = (V.L1[0], V.L1[1] + 0.25, V.L1[2])
    r = nw.NwRenderer(V.scene_l(l1=l1))
    try:
        with pytest.raises(RTError, match="another render"):
            r.progressive(cam, 16, 16, 8, 2, 50, SEED, checkpoint=ck)
    finally:
        r.close()
    r = nw.NwRenderer(V.scene_l())  # (and the same scene built again is accepted)
    try:
        seen = []
        r.progressive(cam, 16, 16, 8, 2, 50, SEED, checkpoint=ck, on_pass=seen.append)
        assert seen == [6, 8]
    finally:
        r.close()


# ---- argument checks ---------------------------------------------------------------------------
def test_argument_checks():
    w = h = 8
    s, cam = nw.preset(2, aspect=1.0)
    r = nw.NwRenderer(s)

    def refused(*a, match=None):
        with pytest.raises(RTError, match=match) as e:
            r.render_pass(cam, *a)
        assert e.value.code == RT_EINVAL

    try:
        refused(w, h, 0, 1, match="rt_nw_accum_reset")  # no accumulator yet
        r.accum_reset(w, h)
        refused(w, h, 1, 1 << 24)  # s_begin + s_count = 2^24 + 1
        refused(w, h, (1 << 24) - 1, 2)
        refused(w, h, 0, -1)
        refused(w, h, -1, 2)
        refused(w + 8, h, 0, 1, match="rt_nw_accum_reset")  # an accumulator of another size
        refused(w, h + 1, 0, 1, match="rt_nw_accum_reset")
        r.render_pass(cam, w, h, 0, 3)
        before, done = r.accum_export()
        assert done == 3 and before.any()
        r.render_pass(cam, w, h, 3, 0)  # nothing to add
        r.render_pass(cam, w, h, 1 << 24, 0)
        after, done = r.accum_export()
        assert done == 3 and np.array_equal(before, after)
        r.accum_reset(w, h)
        r.render_pass(cam, w, h, (1 << 24) - 2, 2)  # the last two samples the RNG key can name
        top, done = r.accum_export()
        assert done == 2 and top.any() and (top >= 0).all()
    finally:
        r.close()


# ---- the CLI -----------------------------------------------------------------------------------
def _cli(args, **kw):
    p = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=300, **kw)
    assert p.returncode == 0, p.stderr
    return p.stderr


@pytest.mark.parametrize("kind", ["scene6", "obj_tumble"])
def test_cli_checkpoint_resume_equals_single_render(kind, tmp_path):
    if not os.access(CLI, os.X_OK):
        pytest.skip("CLI not built")
    if kind == "scene6":
        base = ["--scene", 6, "--width", 48, "--seed", 7]
    else:
        obj = tmp_path / "cube.obj"
        obj.write_text(M.cube_obj("a//n", quads=True, scale=3.0, offset=(5.0, -2.0, 1.0)))
        base = ["--obj", obj, "--obj-copies", 2, "--obj-tumble", "--width", 48, "--height", 32, "--seed", 7]
    ck, a, b, pfm = (str(tmp_path / n) for n in ("c.ckpt", "a.ppm", "b.ppm", "b.pfm"))
    err = _cli(base + ["--spp", 10, "--pass-spp", 5, "--checkpoint", ck, "--out", "/dev/null"])
    assert '"pass_done_spp": 5}' in err and '"pass_done_spp": 10}' in err
    assert nw.accum_info(ck)["spp_done"] == 10
    err = _cli(base + ["--spp", 24, "--pass-spp", 5, "--checkpoint", ck, "--out", b, "--pfm", pfm])
    assert '"pass_done_spp": 15}' in err and '"pass_done_spp": 24}' in err and '"pass_done_spp": 5}' not in err  # resumed at 10
    _cli(base + ["--spp", 24, "--out", a])
    assert open(a, "rb").read() == open(b, "rb").read()
    import a_dive_into_ray_tracing_amd as rt

    mean = rt.read_pfm(pfm)
    assert mean.shape[1] == 48 and np.isfinite(mean).all() and mean.min() >= 0 and mean.max() > 0


def test_cli_time_limit_runs_exactly_one_pass(tmp_path):
    if not os.access(CLI, os.X_OK):
        pytest.skip("CLI not built")
    ck, out, one = (str(tmp_path / n) for n in ("t.ckpt", "t.ppm", "one.ppm"))
    base = ["--scene", 6, "--width", 48, "--seed", 7]
    err = _cli(base + ["--spp", 40, "--pass-spp", 4, "--checkpoint", ck, "--time-limit", 0, "--out", out])
    assert err.count("pass_done_spp") == 1 and '"pass_done_spp": 4}' in err and '"spp": 4,' in err
    assert nw.accum_info(ck)["spp_done"] == 4
    _cli(base + ["--spp", 4, "--out", one])
    assert open(out, "rb").read() == open(one, "rb").read()  # the image of the samples so far
