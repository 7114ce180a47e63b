"""Cost of triangle attributes in the Next-Week renderer: mesh_bench.py's scene
(one icosphere of 320 / 5 120 triangles on the ground sphere, 800x800 at 64
samples per pixel) with the mesh flat under a solid colour, flat under an image
texture (barycentric u, v) and smooth + uv under the same image, alternated
twice, through every closest-hit structure the scene offers.  Prints ms and
Msamples/s (HIP events, the mean of 3 renders after one warm-up).
usage: smooth_bench.py [SUBDIVISIONS ...] (default 2 4)"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import a_dive_into_ray_tracing_amd.nextweek as nw  # noqa: E402
import mesh_bench as B  # noqa: E402

W, H, SPP = 800, 800, int(os.environ.get("SPP", "64"))


def main():
    cam = nw.camera((3.0, 2.0, 4.0), (0, 1, 0), (0, 1, 0), 30, W / H, 0.0, 5.0)
    out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")
    st = torch.cuda.Stream()
    img = np.random.default_rng(1).integers(0, 256, (64, 64, 3)).astype(np.uint8)
    for sub in [int(x) for x in sys.argv[1:]] or [2, 4]:
        v, f = B.icosphere(sub)
        n = v - [0.0, 1.0, 0.0]  # the unit sphere's normals
        uv = np.column_stack([0.5 + 0.5 * n[:, 0], 0.5 + 0.5 * n[:, 1]])
        for rep in (1, 2):
            for mode in ("flat", "flat_image", "smooth_uv_image"):
                s = nw.Scene()
                tex = s.solid(0.7, 0.35, 0.2) if mode == "flat" else s.image(img)
                kw = dict(normals=n, uvs=uv, smooth=True) if mode == "smooth_uv_image" else {}
                s.add(s.mesh(v, f, mat=s.lambertian(tex), **kw))
                s.add(s.sphere((0, -1000, 0), 1000, s.lambertian(s.checker(s.solid(0.2, 0.3, 0.1), s.solid(0.9, 0.9, 0.9)))))
                s.set_background(0.7, 0.8, 1.0)
                r = nw.NwRenderer(s)
                for accel in ("grid", "bvh"):
                    r.set_accel(accel)
                    if r.accel_info()["accel"] != accel:
                        continue
                    r.render_rows(cam, W, H, SPP, 50, 1984, 0, 1, H, out.data_ptr(), st.cuda_stream)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    for _ in range(3):
                        r.render_rows(cam, W, H, SPP, 50, 1984, 0, 1, H, out.data_ptr(), st.cuda_stream)
                    e1.record(st)
                    torch.cuda.synchronize()
                    ms = e0.elapsed_time(e1) / 3
                    k = r.last_kernel()
                    print(f"{len(f)} triangles run {rep} {mode:16s} {accel}: {ms:.2f} ms, {W * H * SPP / ms / 1e3:.0f} Msamples/s, "
                          f"{r.last_segments() / (W * H * SPP):.2f} segments/sample "
                          f"({'persistent' if k['persistent'] else 'one-shot'})", flush=True)
                r.close()


if __name__ == "__main__":
    main()
