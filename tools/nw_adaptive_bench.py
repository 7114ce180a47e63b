"""Measurements of adaptive sampling in the Next-Week renderer (profiles/adaptive/README.md); one GPU.

  python tools/nw_adaptive_bench.py [--out FILE.json] [--only cost,gain,estimate]

  cost      an all-active rt_nw_adapt_pass against rt_nw_render_pass of the same size, on the final scene and on the
            motion-blur scene: what the list decode and the fourth accumulator cost;
  gain      presets 6 and 8: an adaptive render at a threshold against a uniform render of the same total sample
            count — RMSE against a high-spp render of another seed, and wall time;
  estimate  preset 6, 32 x 32 x 256: mean over pixels of the estimated variance of the mean, per seed, over the
            empirical variance of the pixel means across 32 seeds (the band of tests/test_nw_adaptive_gpu.py).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import a_dive_into_ray_tracing_amd.nextweek as nw  # noqa: E402

SEED = 1984


def timed(fn, sync, rounds=3):
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def cost(res):
    earth = nw.load_image(os.path.join(REPO, "tests", "golden", "earthmap.jpeg"))
    for name, which, w, h, spp in (("final", 8, 800, 800, 1024), ("motion_blur", 1, 1200, 800, 500)):
        s, cam = nw.preset(which, image=earth, aspect=w / h)
        r = nw.NwRenderer(s)
        r.accum_reset(w, h)
        r.adapt_reset(w, h)
        r.render_pass(cam, w, h, 0, spp, 50, SEED)  # warm-up
        r.last_segments()
        plain, adapt = [], []
        for k in range(3):  # alternated
            plain += timed(lambda: r.render_pass(cam, w, h, 0, spp, 50, SEED), r.last_segments, 1)
            r.adapt_reset(w, h)
            adapt += timed(lambda: r.adapt_pass(cam, w, h, spp, 50, SEED), r.last_segments, 1)
        kern = r.last_kernel()
        r.close()
        res["cost_" + name] = {"size": [w, h, spp], "render_pass_ms": plain, "adapt_pass_ms": adapt, "kernel": kern,
                               "ratio_of_medians": float(np.median(adapt) / np.median(plain))}
        print("cost", name, res["cost_" + name], flush=True)


def gain(res):
    for which, w, h, lo, hi, pass_spp, thr, ref_spp in ((6, 256, 256, 64, 2048, 64, 0.05, 16384), (8, 256, 256, 64, 2048, 64, 0.03, 16384)):
        s, cam = nw.preset(which, image=nw.load_image(os.path.join(REPO, "tests", "golden", "earthmap.jpeg")), aspect=w / h)
        r = nw.NwRenderer(s)
        ref = r.render(cam, w, h, ref_spp, 50, SEED + 1) / np.float32(ref_spp)
        r.adaptive(cam, w, h, lo, hi, pass_spp, thr, seed=SEED)  # warm-up
        st = {}
        t0 = time.perf_counter()
        mean, n, _ = r.adaptive(cam, w, h, lo, hi, pass_spp, thr, seed=SEED, stats=st)
        t_adapt = (time.perf_counter() - t0) * 1e3
        spp = int(round(st["total_samples"] / (w * h)))
        r.render(cam, w, h, spp, 50, SEED)
        t0 = time.perf_counter()
        uni = r.render(cam, w, h, spp, 50, SEED) / np.float32(spp)
        t_uni = (time.perf_counter() - t0) * 1e3
        r.close()

        def rmse(a):
            d = a.astype(np.float64) - ref
            return float(np.sqrt((d * d).mean())), float(np.sqrt(((d / (ref + 0.01)) ** 2).mean()))

        res["gain_preset%d" % which] = {
            "size": [w, h], "min_max_pass_threshold": [lo, hi, pass_spp, thr], "passes": st["passes"],
            "total_samples": st["total_samples"], "mean_spp": st["total_samples"] / (w * h), "uniform_spp": spp,
            "share_at_max": st["pixels_at_max"] / (w * h), "share_at_min": float((n == lo).mean()),
            "adaptive_ms": t_adapt, "uniform_ms": t_uni, "rmse_abs_rel_adaptive": rmse(mean), "rmse_abs_rel_uniform": rmse(uni),
            "reference_spp": ref_spp}
        print("gain", which, res["gain_preset%d" % which], flush=True)


def estimate(res):
    w = h = 32
    spp, seeds = 256, 32
    s, cam = nw.preset(6, aspect=1.0)
    r = nw.NwRenderer(s)
    means = np.stack([r.render(cam, w, h, spp, 50, 1000 + k).astype(np.float64).sum(axis=2) / spp for k in range(seeds)])
    emp = means.var(axis=0, ddof=1).mean()
    ratios = []
    for k in range(16):
        r.adapt_reset(w, h)
        r.adapt_pass(cam, w, h, spp, 50, 1000 + k)
        sm, m2, n = r.adapt_export()
        mean = sm.sum(axis=2).astype(np.float64) * 2.0 ** -32 / n
        var = np.maximum(0.0, m2.astype(np.float64) * 2.0 ** -28 / n - mean * mean) * n / (n - 1.0)
        ratios.append(float((var / n).mean() / emp))
    r.close()
    res["estimate"] = {"empirical_variance_of_the_mean": float(emp), "ratios_seeds_1000_1015": ratios, "min": min(ratios),
                       "max": max(ratios), "mean": float(np.mean(ratios)), "std": float(np.std(ratios, ddof=1))}
    print("estimate", res["estimate"], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the results to this JSON file")
    ap.add_argument("--only", default="cost,gain,estimate")
    a = ap.parse_args()
    res = {}
    for name in a.only.split(","):
        {"cost": cost, "gain": gain, "estimate": estimate}[name](res)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
