"""What a group film costs beside the single-context film (a tool, not a test; bench.py is the
contract benchmark).  One process, one device; groups with repeated entries ([0], [0, 0, 0, 0]) run
the multi-device path on it, so on one GPU the figures measure OVERHEAD, not scaling: four contexts
share the device the single film has to itself.

On the final scene at 1920x1080, depth 50, after a warm-up chunk of every film:

  accumulate   one 64-spp chunk: the plain ykgpu_film_accumulate, a one-entry group film (the same
               launches plus the group's host bookkeeping) and a four-entry group film; every round
               renders the same samples [64 r, 64 r + 64) on each
  guided       ykgpu_film_denoise_guided at the defaults, RGB8 only, on the films as they stand after
               the chunks: the call's wall clock and its stats (for a group film each device time is
               the largest entry's, and exchange_ms is shown apart)
  denoise      the colour-only filter, the same way

The variants alternate round by round, so a drift of the device shows in all of them; each figure is
the median of --runs rounds with the minimum and maximum beside it.  The films are compared at the
end: sums, second moments and both filtered images must be bit-equal.

usage: python tools/group_film_bench.py [--runs 7] [--width 1920] [--chunk 64] [--out profiles/TAG_group_film.json]
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
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--scene", default="final")
    ap.add_argument("--entries", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs must be at least 5")
    arr, cam = yk.build_scene(a.scene, 42)
    p = make_params(a.width, None, a.chunk * (a.runs + 1), a.depth, 404)
    names = ["film", "group1", f"group{a.entries}"]
    with yk.Renderer(0) as ren, yk.Group([0]) as g1, yk.Group([0] * a.entries) as gk:
        for owner in (ren, g1, gk):
            owner.set_scene(arr, cam)
        films = dict(zip(names, (ren.film(p), g1.film(p), gk.film(p))))

        def chunk(f):
            t = time.perf_counter()
            f.accumulate(a.chunk)
            return (time.perf_counter() - t) * 1e3

        def filt(f, guided):
            t = time.perf_counter()
            _, rgb, st = f.denoise_guided(want_mean=False) if guided else f.denoise(want_mean=False)
            return (time.perf_counter() - t) * 1e3, st, rgb

        acc = {n: [] for n in names}
        for f in films.values():  # warm-up: code objects, ring allocations
            chunk(f)
        for r in range(a.runs):
            order = names if r % 2 == 0 else names[::-1]
            for n in order:
                acc[n].append(chunk(films[n]))
        kernel = {"film": ren.stats()["kernel_ms"], "group1": g1.stats(-1)["kernel_ms"],
                  f"group{a.entries}": gk.stats(-1)["kernel_ms"]}
        state = {n: f.read() for n, f in films.items()}
        equal = all(s[0].tobytes() == state["film"][0].tobytes() and s[1].tobytes() == state["film"][1].tobytes() and
                    s[2] == state["film"][2] for s in state.values())
        del state
        filters = {}
        for guided in (True, False):
            wall = {n: [] for n in names}
            stats = {n: [] for n in names}
            images = {}
            for f in films.values():  # warm-up: the buffers, the feature pass
                filt(f, guided)
            for r in range(a.runs):
                order = names if r % 2 == 0 else names[::-1]
                for n in order:
                    ms, st, images[n] = filt(films[n], guided)
                    wall[n].append(ms)
                    stats[n].append(st)
            equal = equal and all(img.tobytes() == images["film"].tobytes() for img in images.values())
            filters["guided" if guided else "denoise"] = {
                n: dict(summary(wall[n]), **{k: summary([s[k] for s in stats[n]]) for k in stats[n][0] if k != "total_ms"})
                for n in names}
        for f in films.values():
            f.close()
    lo, hi = min(acc["film"]), max(acc["film"])
    out = {
        "tool": "tools/group_film_bench.py", "scene": a.scene, "width": a.width, "height": p.image_height,
        "chunk_spp": a.chunk, "depth": a.depth, "entries": a.entries,
        "timing": "host wall clock around synchronous calls, median of alternating rounds; one GPU: overhead, not scaling",
        "bit_equal": equal,
        "accumulate": {n: dict(summary(v), last_kernel_ms=round(kernel[n], 3)) for n, v in acc.items()},
        "group1_median_inside_film_spread": bool(lo <= statistics.median(acc["group1"]) <= hi),
        "filters_rgb8_only": filters,
    }
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
