"""Shared meshes against flattened copies in the Next-Week renderer: an N x N
field (N = 1, 4, 16) of one icosphere of 5 120 or 81 920 triangles (radius 1,
lambertian) standing on a ground plane (the R = 1000 sphere) under the sky
background, 800x800 at 64 samples per pixel.  Every case is built twice — the
mesh placed through Scene.shared (one pool, one record per placement, the
two-level walk) and without it (one leaf record per triangle per placement,
today's BVH) — and the two are rendered alternately in the same process.
Prints per build: ms and Msamples/s (HIP events, the mean of 3 renders after
one warm-up), segments per sample, the scene's set-up time (flatten + BVH build
+ upload), the device bytes of records and nodes, the kernel and what it walked
from LDS; and whether the two images are equal.  An unshared build of more than
MAX_UNSHARED triangles (default 2 000 000) is not attempted: its host BVH
build alone takes minutes.
usage: instance_bench.py [SUBDIVISIONS ...] (default 4 6); env SPP, FIELDS
(default "1 4 16"), MAX_UNSHARED, SHARED_ONLY=1

--move: moving placements (Scene.move) against the static shared build of the
same field (FIELDS default "4 16"), three builds rendered alternately: "static"
(Scene.shared as above; it must stay on the TRI = 3 kernels), "moving" (every
placement moves by MOVE = (0.3, 0.4, 0), 0.5 units, over the shutter [0, 1]:
TRI = 4, swept top-level boxes) and "at rest" (every placement under Scene.move
with offset0 == offset1: TRI = 4, the static build's boxes and image).  With
the work-counting build (RTMI_LIBRARY=.../librtmi_stats.so) one more render per
build prints its node visits and triangle tests per sample.

--tumble: affine placements (Scene.transform) against the rotate_y fields, three
builds rendered alternately (FIELDS default "4 16"): "rotate_y" (the static
shared field: TRI = 3), "same as affine" (every copy's rotate_y + translate
written as one 3 x 4 matrix: the same geometry through the TRI = 5 kernels and
the 3 x 3 entry — what that entry costs) and "tumbled" (the CLI's --obj-tumble:
scaled by 0.75 + 0.25 sin(2.9 q), turned 37 q degrees about a skew axis, stood
on the ground: TRI = 5).  Counters as for --move."""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import a_dive_into_ray_tracing_amd.nextweek as nw  # noqa: E402
from mesh_bench import icosphere  # noqa: E402

W, H, SPP = 800, 800, int(os.environ.get("SPP", "64"))
MOVING = "--move" in sys.argv
TUMBLE = "--tumble" in sys.argv
MOVE = (0.3, 0.4, 0.0)
FIELDS = [int(x) for x in os.environ.get("FIELDS", "4 16" if MOVING or TUMBLE else "1 4 16").split()]
MAX_UNSHARED = int(os.environ.get("MAX_UNSHARED", "2000000"))
SHARED_ONLY = os.environ.get("SHARED_ONLY") == "1"


def build(v, f, n, shared, move=None, affine=None):
    """The field: copy (i, k) 3 units from its neighbours, turned by 37 q
    degrees and nudged (q = i n + k), as the CLI's --obj-copies places them.
    move: every placement under Scene.move from (0, 0, 0) to that vector.
    affine "same": the placement as one Scene.transform matrix; "tumbled": the
    CLI's --obj-tumble map (the mesh here fills [-1, 1]^3 about its centre (0, 1, 0))."""
    s = nw.Scene()
    mesh = s.mesh(v, f, mat=s.lambertian(s.solid(0.7, 0.35, 0.2)))
    h = s.shared(mesh) if shared else mesh
    for i in range(n):
        for k in range(n):
            q = i * n + k
            off = (3.0 * (i - 0.5 * (n - 1)) + 0.4 * np.sin(1.7 * q), 0.0, 3.0 * (k - 0.5 * (n - 1)) + 0.4 * np.cos(2.3 * q))
            if affine == "same":
                placed = s.transform(h, nw.affine(angle=37.0 * q, translate=off))
            elif affine == "tumbled":
                m = nw.affine(scale=0.75 + 0.25 * np.sin(2.9 * q), axis=(np.sin(1.3 * q), 1.0, np.cos(0.7 * q)), angle=37.0 * q)
                corners = np.array([[x, y, z] for x in (-1, 1) for y in (0, 2) for z in (-1, 1)], np.float64)
                m[:, 3] = (off[0], off[1] - (corners @ m[:, :3].T)[:, 1].min(), off[2])
                placed = s.transform(h, m)
            else:
                placed = s.translate(s.rotate_y(h, 37.0 * q), off)
            s.add(placed if move is None else s.move(placed, (0, 0, 0), move))
    s.add(s.sphere((0, -1000, 0), 1000, s.lambertian(s.checker(s.solid(0.2, 0.3, 0.1), s.solid(0.9, 0.9, 0.9)))))
    s.set_background(0.7, 0.8, 1.0)
    return s


def counters():
    """{node visits, object tests} since the last call, or None in the product build."""
    import ctypes as C

    from a_dive_into_ray_tracing_amd._abi import load

    v = (C.c_uint64 * 4)()
    return None if load().rt_nw_debug_counters(v) != 0 else (v[1], v[2])


def main_move():
    out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")
    st = torch.cuda.Stream()
    cases = ((("rotate_y", None, 3), ("same as affine", "same", 5), ("tumbled", "tumbled", 5)) if TUMBLE else
             (("static", None, 3), ("moving", MOVE, 4), ("at rest", (0, 0, 0), 4)))
    for sub in [int(x) for x in sys.argv[1:] if not x.startswith("--")] or [4, 6]:
        v, f = icosphere(sub)
        for n in FIELDS:
            back = 1.0 if n == 1 else 0.5 + 0.75 * n
            cam = nw.camera((3.0 * back, 1.0 + 1.0 * back, 4.0 * back), (0, 1, 0), (0, 1, 0), 30, W / H, 0.0, 5.0 * back)
            runs = {}
            for name, move, tri in cases:
                s = build(v, f, n, True, affine=move) if TUMBLE else build(v, f, n, True, move)
                r = nw.NwRenderer(s)
                assert r.scene_tri() == tri, (name, r.scene_tri())
                r.render_rows(cam, W, H, SPP, 50, 1984, 0, 1, H, out.data_ptr(), st.cuda_stream)  # warm-up
                torch.cuda.synchronize()
                runs[name] = dict(r=r, ms=[], img=out.cpu().numpy().copy(), nodes=s.instancing_stats()["top_nodes"])
            for _ in range(3):  # alternating
                for name, q in runs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    q["r"].render_rows(cam, W, H, SPP, 50, 1984, 0, 1, H, out.data_ptr(), st.cuda_stream)
                    e1.record(st)
                    torch.cuda.synchronize()
                    q["ms"].append(e0.elapsed_time(e1))
            head = f"{len(f)} triangles x {n}x{n}"
            for name, q in runs.items():
                r, ms = q["r"], float(np.mean(q["ms"]))
                k, g = r.last_kernel(), r.last_staging()
                work = ""
                if counters() is not None:  # (zeroed by the call) one more render, counted
                    r.render_rows(cam, W, H, SPP, 50, 1984, 0, 1, H, out.data_ptr(), st.cuda_stream)
                    torch.cuda.synchronize()
                    nv, ot = counters()
                    work = f", {nv / (W * H * SPP):.2f} node visits/sample, {ot / (W * H * SPP):.2f} object tests/sample"
                print(f"{head} {name}: {ms:.2f} ms ({min(q['ms']):.2f}..{max(q['ms']):.2f}), {W * H * SPP / ms / 1e3:.0f} Msamples/s, "
                      f"{r.last_segments() / (W * H * SPP):.3f} segments/sample{work}, TRI = {r.scene_tri()}, {q['nodes']} top-level nodes "
                      f"({'persistent' if k['persistent'] else 'one-shot'} kernel, chunk {k['chunk']}, "
                      f"top nodes {'LDS' if g['nodes_lds'] else 'global'}, top records {'LDS' if g['objects_lds'] else 'global'})",
                      flush=True)
                r.close()
            if TUMBLE:
                same = np.array_equal(runs["rotate_y"]["img"], runs["same as affine"]["img"])
                diff = np.abs(runs["rotate_y"]["img"] - runs["same as affine"]["img"])
                print(f"{head}: the same field through affine placements {'equals' if same else 'differs from'} the rotate_y image "
                      f"({(diff > 0).any(axis=2).mean():.4f} of the pixels, mean |difference| {diff.mean():.2e} of a mean {runs['rotate_y']['img'].mean():.3f})",
                      flush=True)
                continue
            print(f"{head}: at rest image {'equals' if np.array_equal(runs['static']['img'], runs['at rest']['img']) else 'DIFFERS from'} "
                  f"the static one; moving image {'equals' if np.array_equal(runs['static']['img'], runs['moving']['img']) else 'differs from'} it",
                  flush=True)


def main():
    if MOVING or TUMBLE:
        return main_move()
    out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")
    st = torch.cuda.Stream()
    for sub in [int(x) for x in sys.argv[1:]] or [4, 6]:
        v, f = icosphere(sub)
        for n in FIELDS:
            back = 1.0 if n == 1 else 0.5 + 0.75 * n
            cam = nw.camera((3.0 * back, 1.0 + 1.0 * back, 4.0 * back), (0, 1, 0), (0, 1, 0), 30, W / H, 0.0, 5.0 * back)
            runs = {}
            for name, shared in (("shared", True), ("unshared", False)):
                if not shared and (SHARED_ONLY or len(f) * n * n > MAX_UNSHARED):
                    continue
                t0 = time.time()
                s = build(v, f, n, shared)
                r = nw.NwRenderer(s)
                setup = time.time() - t0
                prims, nodes = r.info()
                if shared:
                    q = s.instancing_stats()
                    dev = (q["top_leaves"] + q["pool_triangles"]) * 52 + (q["top_nodes"] + q["bottom_nodes"]) * 32
                else:
                    dev = prims * 52 + nodes * 32
                r.set_accel("bvh")
                r.render_rows(cam, W, H, SPP, 50, 1984, 0, 1, H, out.data_ptr(), st.cuda_stream)  # warm-up
                torch.cuda.synchronize()
                runs[name] = dict(r=r, setup=setup, dev=dev, ms=[], img=out.cpu().numpy().copy())
            for _ in range(3):  # alternating
                for name, q in runs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    q["r"].render_rows(cam, W, H, SPP, 50, 1984, 0, 1, H, out.data_ptr(), st.cuda_stream)
                    e1.record(st)
                    torch.cuda.synchronize()
                    q["ms"].append(e0.elapsed_time(e1))
            head = f"{len(f)} triangles x {n}x{n}"
            for name, q in runs.items():
                r, ms = q["r"], float(np.mean(q["ms"]))
                k, g = r.last_kernel(), r.last_staging()
                print(f"{head} {name}: {ms:.2f} ms ({min(q['ms']):.2f}..{max(q['ms']):.2f}), {W * H * SPP / ms / 1e3:.0f} Msamples/s, "
                      f"{r.last_segments() / (W * H * SPP):.2f} segments/sample, set-up {q['setup']:.2f} s, "
                      f"{q['dev'] / 1e6:.2f} MB of records and nodes "
                      f"({'persistent' if k['persistent'] else 'one-shot'} kernel, chunk {k['chunk']}, "
                      f"top nodes {'LDS' if g['nodes_lds'] else 'global'}, top records {'LDS' if g['objects_lds'] else 'global'})",
                      flush=True)
                r.close()
            if len(runs) == 2:
                print(f"{head}: images {'equal' if np.array_equal(runs['shared']['img'], runs['unshared']['img']) else 'DIFFER'}",
                      flush=True)
            else:
                print(f"{head}: unshared build not attempted ({len(f) * n * n} triangles)", flush=True)


if __name__ == "__main__":
    main()
