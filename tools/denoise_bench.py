"""What the film's denoise filter costs (a tool, not a test; bench.py is the contract benchmark).

On BASELINE config 3's image (final scene, 1920x1080, depth 50) with a film of 64 samples per pixel
it times, in one process on one device after a warm-up of every shape, as host wall clock around
synchronous calls:

  chunk_64spp      one ykgpu_film_accumulate of 64 samples into the emptied film: the chunk a
                   denoised preview previews, and the comparison for everything below
  denoise_rgb      ykgpu_film_denoise at the defaults (R = 5, F = 1) with the RGB8 image only
  denoise_rgb_mean ... with the float64 mean copied out as well (24 B per pixel)
  denoise_r3       ... RGB8 only at R = 3
  denoise_r10      ... RGB8 only at R = 10

and records, per denoise variant, the call's own device times (yk_denoise_stats: moments_ms for
yk_film_moments, filter_ms for yk_film_nlm and the RGB8 conversion, between events on the stream).
The variants alternate round by round, so a drift of the device shows in all of them; each figure
is the median of --runs rounds, with the minimum and maximum beside it.  `preview_over_chunk` is
(moments_ms + filter_ms) at the defaults over the chunk's wall clock: the goal is below 0.5.

usage: python tools/denoise_bench.py [--runs 7] [--width 1920] [--spp 64] [--out profiles/TAG_denoise.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uecraytracing_amd as yk  # noqa: E402
from uecraytracing_amd.records import make_params  # noqa: E402


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "runs": len(ms), "ms": [round(x, 3) for x in ms]}


VARIANTS = {
    "denoise_rgb": dict(want_mean=False),
    "denoise_rgb_mean": dict(),
    "denoise_r3": dict(radius=3, want_mean=False),
    "denoise_r10": dict(radius=10, want_mean=False),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--scene", default="final")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs must be at least 5")
    arr, cam = yk.build_scene(a.scene, 42)
    p = make_params(a.width, None, a.spp, a.depth, 404)
    wall = {"chunk_%dspp" % a.spp: []}
    wall.update({k: [] for k in VARIANTS})
    dev = {k: {"moments_ms": [], "filter_ms": []} for k in VARIANTS}
    with yk.Renderer(0) as ren:
        ren.set_scene(arr, cam)
        film = ren.film(p)
        zero = film.read()

        def chunk():
            film.write(zero[0], zero[1], 0)
            t = time.perf_counter()
            film.accumulate(a.spp)
            return (time.perf_counter() - t) * 1e3

        def denoise(kw):
            t = time.perf_counter()
            _, _, st = film.denoise(**kw)
            return (time.perf_counter() - t) * 1e3, st

        # warm-up: every shape once (code objects, the film's denoise buffers, the launch rings)
        chunk()
        for kw in VARIANTS.values():
            denoise(kw)
        for _ in range(a.runs):
            wall["chunk_%dspp" % a.spp].append(chunk())
            for name, kw in VARIANTS.items():
                ms, st = denoise(kw)
                wall[name].append(ms)
                for k in dev[name]:
                    dev[name][k].append(st[k])
        film.close()
    base = statistics.median(wall["chunk_%dspp" % a.spp])
    calls = {}
    for name, ms in wall.items():
        calls[name] = summary(ms)
        if name in dev:
            calls[name]["moments_ms"] = summary(dev[name]["moments_ms"])
            calls[name]["filter_ms"] = summary(dev[name]["filter_ms"])
            calls[name]["device_over_chunk"] = round(
                (statistics.median(dev[name]["moments_ms"]) + statistics.median(dev[name]["filter_ms"])) / base, 4)
    out = {
        "tool": "tools/denoise_bench.py", "scene": a.scene, "width": a.width, "height": p.image_height, "spp": a.spp,
        "depth": a.depth,
        "timing": "host wall clock around synchronous calls; moments_ms / filter_ms between events on the stream; "
                  "medians of alternating rounds",
        "calls": calls,
        "preview_over_chunk": calls["denoise_rgb"]["device_over_chunk"],
    }
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
