"""What the progressive film costs (a tool, not a test; bench.py is the contract benchmark).

On BASELINE config 3 (final scene, 1920x1080, 512 spp, depth 50) it times, in one process on one
device after a warm-up of every shape, as host wall clock around synchronous calls:

  one_shot       Renderer.render_sums: the comparison for everything below (it ends with the copy
                 of the float64 sums, 24 B per pixel, to the host)
  one_shot_rgb   Renderer.render: the same call ending with the RGB8 copy (3 B per pixel) instead
  film_1x512     a film filled in one chunk: the same launches, each folded by yk_film_reduce
                 (6 accumulators per pixel, read and written every launch) instead of
                 yk_reduce_samples (3, through ctx->d_acc)
  film_8x64      a film filled in 8 chunks of 64 \\ every chunk is a synchronous call with its own
  film_32x16     ... in 32 chunks of 16          / ramp (4, 8, 16, ...) and drain
  error          one ykgpu_film_error without the map (count and maximum only), and with it
  resolve        one ykgpu_film_resolve

The variants alternate round by round (one_shot, one_shot_rgb, film_1x512, film_8x64, film_32x16, one_shot, ...),
so a drift of the device shows in all of them; each figure is the median of --runs rounds, with
the minimum and maximum beside it (the spread of the box).  The filled films are compared with the
one-shot sums: they must be bit-equal at this size too.

usage: python tools/film_bench.py [--runs 7] [--width 1920] [--spp 512] [--out profiles/TAG_film.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=512)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--scene", default="final")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs must be at least 5")
    arr, cam = yk.build_scene(a.scene, 42)
    p = make_params(a.width, None, a.spp, a.depth, 404)
    chunkings = {f"film_1x{a.spp}": [a.spp]}
    for n in (8, 32):
        if a.spp % n == 0 and a.spp // n >= 1:
            chunkings[f"film_{n}x{a.spp // n}"] = [a.spp // n] * n
    times = {"one_shot": [], "one_shot_rgb": []}
    times.update({k: [] for k in chunkings})
    launches = {}
    with yk.Renderer(0) as ren:
        ren.set_scene(arr, cam)
        film = ren.film(p)
        zero = film.read()

        def one_shot():
            t = time.perf_counter()
            sums = ren.render_sums(p)
            return (time.perf_counter() - t) * 1e3, sums

        def one_shot_rgb():
            t = time.perf_counter()
            ren.render(p)
            return (time.perf_counter() - t) * 1e3

        def fill(chunks):
            film.write(zero[0], zero[1], 0)
            n = 0
            t = time.perf_counter()
            for c in chunks:
                film.accumulate(c)
                n += ren.stats()["launches"]
            return (time.perf_counter() - t) * 1e3, n

        # warm-up: every shape once (code objects, ring allocations of each launch size)
        _, want = one_shot()
        launches["one_shot"] = launches["one_shot_rgb"] = ren.stats()["launches"]
        one_shot_rgb()
        equal = True
        for name, chunks in chunkings.items():
            _, launches[name] = fill(chunks)
            equal = equal and film.read()[0].tobytes() == want.tobytes()
        for _ in range(a.runs):
            times["one_shot"].append(one_shot()[0])
            times["one_shot_rgb"].append(one_shot_rgb())
            for name, chunks in chunkings.items():
                times[name].append(fill(chunks)[0])
        # the film is full: the error map and the resolve at done == spp
        err, err_map, res = [], [], []
        film.error(0.0, want_map=True), film.resolve()
        for _ in range(a.runs):
            t = time.perf_counter()
            _, st = film.error(1e-6, want_map=False)
            err.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            film.error(1e-6, want_map=True)
            err_map.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            film.resolve()
            res.append((time.perf_counter() - t) * 1e3)
        film.close()
    base = statistics.median(times["one_shot"])
    out = {
        "tool": "tools/film_bench.py", "scene": a.scene, "width": a.width, "height": p.image_height, "spp": a.spp,
        "depth": a.depth, "timing": "host wall clock around synchronous calls, median of alternating rounds",
        "film_sums_bit_equal_to_one_shot": equal,
        "calls": {k: dict(summary(v), launches=launches[k], over_one_shot=round(statistics.median(v) / base, 4))
                  for k, v in times.items()},
        "error_stats_only": summary(err), "error_with_map": summary(err_map), "resolve": summary(res),
        "error_at_1e-6": st,
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
