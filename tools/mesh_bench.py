"""Baseline of the Next-Week renderer's triangle meshes: one icosphere of 320,
5 120 and 81 920 triangles (radius 1, lambertian) standing on a ground plane
(the R = 1000 sphere) under the sky background, 800x800 at 64 samples per
pixel, through every closest-hit structure the scene offers.  Prints
Msamples/s (HIP events, the mean of 3 renders after one warm-up), the kernel
(rt_nw_ctx_last_kernel) and what it walked from LDS (rt_nw_ctx_last_staging).
usage: mesh_bench.py [SUBDIVISIONS ...] (default 2 4 6)"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import a_dive_into_ray_tracing_amd.nextweek as nw  # noqa: E402

W, H, SPP = 800, 800, int(os.environ.get("SPP", "64"))


def icosphere(subdiv):
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [np.array(x, np.float64) for x in ((-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p),
                                           (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1))]
    v = [x / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) + [0.0, 1.0, 0.0], np.array(f, np.int32)


def main():
    cam = nw.camera((3.0, 2.0, 4.0), (0, 1, 0), (0, 1, 0), 30, W / H, 0.0, 5.0)
    out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")
    st = torch.cuda.Stream()
    for sub in [int(x) for x in sys.argv[1:]] or [2, 4, 6]:
        s = nw.Scene()
        v, f = icosphere(sub)
        s.add(s.mesh(v, f, mat=s.lambertian(s.solid(0.7, 0.35, 0.2))))
        s.add(s.sphere((0, -1000, 0), 1000, s.lambertian(s.checker(s.solid(0.2, 0.3, 0.1), s.solid(0.9, 0.9, 0.9)))))
        s.set_background(0.7, 0.8, 1.0)
        t0 = time.time()
        r = nw.NwRenderer(s)
        build_s = time.time() - t0
        prims, nodes = r.info()
        line = [f"{len(f)} triangles ({nodes} BVH nodes, scene set in {build_s:.2f} s):"]
        for accel in ("grid", "bvh"):
            r.set_accel(accel)
            if r.accel_info()["accel"] != accel:
                line.append(f"{accel} (none for this scene)")
                continue
            r.render_rows(cam, W, H, SPP, 50, 1984, 0, 1, H, out.data_ptr(), st.cuda_stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(3):
                r.render_rows(cam, W, H, SPP, 50, 1984, 0, 1, H, out.data_ptr(), st.cuda_stream)
            e1.record(st)
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / 3
            k, g = r.last_kernel(), r.last_staging()
            line.append(f"{accel} {ms:.2f} ms, {W * H * SPP / ms / 1e3:.0f} Msamples/s, "
                        f"{r.last_segments() / (W * H * SPP):.2f} segments/sample "
                        f"({'persistent' if k['persistent'] else 'one-shot'} kernel, chunk {k['chunk']}, "
                        f"nodes {'LDS' if g['nodes_lds'] else 'global' if not k['grid'] else '-'}, "
                        f"objects {'LDS' if g['objects_lds'] else 'global'})")
        r.close()
        print(" | ".join(line), flush=True)


if __name__ == "__main__":
    main()
