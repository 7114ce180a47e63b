"""The host cost of one Next-Week launch (needs the GPU): the wall time of
rt_nw_render_pass plus a stream synchronize on a toy render — preset 1 at
64 x 64 pixels, one sample per pass — where the kernel is a few microseconds
and what remains is the launch path itself (shape, kernel choice, attribute
and occupancy lookups, the memsets, the launch).

    python tools/nw_launch_cost.py [--calls 2000] [--warmup 200]

prints one JSON line: the median, the quartiles and the extremes in microseconds
per call.  RTMI_LIBRARY chooses the library, as everywhere."""
import argparse
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import a_dive_into_ray_tracing_amd.nextweek as nw  # noqa: E402


def loaded_hip():
    """The HIP runtime the library itself runs on (a second copy found by name may be another version)."""
    with open("/proc/self/maps") as f:
        for ln in f:
            if "libamdhip64.so" in ln:
                return C.CDLL(ln.split()[-1])
    raise RuntimeError("the library has not loaded libamdhip64")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    args = ap.parse_args()
    W = H = 64
    s, cam = nw.preset(1, aspect=1.0)
    r = nw.NwRenderer(s)
    hip = loaded_hip()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        r.accum_reset(W, H)
        t = []
        for k in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            r.render_pass(cam, W, H, k, 1, 50, 1984, stream=stream.value)
            rc = hip.hipStreamSynchronize(stream)
            t1 = time.perf_counter()
            assert rc == 0, rc
            if k >= args.warmup:
                t.append((t1 - t0) * 1e6)
        kernel = r.last_kernel()
    finally:
        r.close()
        hip.hipStreamDestroy(stream)
    t.sort()
    q = lambda f: round(t[min(len(t) - 1, int(f * len(t)))], 2)  # noqa: E731
    print(json.dumps({"metric": "nw_launch_cost_us", "median": q(0.5), "p25": q(0.25), "p75": q(0.75), "min": round(t[0], 2),
                      "max": round(t[-1], 2), "calls": len(t), "warmup": args.warmup, "kernel": kernel,
                      "library": os.environ.get("RTMI_LIBRARY", "lib/librtmi.so")}))


if __name__ == "__main__":
    main()
