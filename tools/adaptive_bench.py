"""What adaptive film passes cost and save (a tool, not a test; bench.py is the contract benchmark).

On BASELINE config 3 (final scene, 1920x1080, target 512 spp, depth 50, chunks of 64) it brings a
film to one common error bound by two routes, in one process on one device after a warm-up of
both, timed as host wall clock around synchronous calls:

  uniform    the progressive film's route: ykgpu_film_accumulate chunks for every pixel, and after
             each a ykgpu_film_error, until no pixel is over the bound (or the target is reached)
  adaptive   ykgpu_film_accumulate_adaptive passes at the bound until one selects nothing: the
             first is a uniform chunk, every later one samples only the pixels still over it

The bound (--until, a standard error; threshold2 = until**2) defaults to the largest e2 of the
frame at the target, found in the warm-up: the loosest bound the uniform route meets only with its
last chunk, so the whole frame pays the sample count of its worst pixel.

The context's rings follow its calls (grown when a call needs more, given back when it needs less
than half), and a reallocation of the frame's multi-GB rings costs more than either route.  So
before each timed route one untimed full-frame chunk sizes the rings for the route's first call,
as they are in a process that has rendered a frame before; what the adaptive route's shrinking
groups then do to the rings is part of its time.

The routes alternate round by round; each figure is the median of --runs rounds with the minimum
and maximum beside it.  Per adaptive pass it records pixels selected, samples, groups, launches,
wall ms and the part of it with no path-tracing launch running (wall - render_busy_ms: selection,
compaction, the synchronisation between groups, ring reallocation, each group's ramp and drain).
select_ms is a pass that selects nothing (threshold +inf): the selection kernel and its read-back
alone.  ms per million samples compares what a sample costs on each route.

usage: python tools/adaptive_bench.py [--runs 7] [--width 1920] [--spp 512] [--chunk 64] [--until X]
                                      [--out profiles/TAG_adaptive.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uecraytracing_amd as yk  # noqa: E402
from uecraytracing_amd.records import make_params  # noqa: E402


def summary(v, nd=3):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd), "runs": len(v),
            "all": [round(x, nd) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--scene", default="final")
    ap.add_argument("--until", type=float, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    arr, cam = yk.build_scene(a.scene, 42)
    p = make_params(a.width, None, a.spp, a.depth, 404)
    npix = p.image_width * p.image_height
    with yk.Renderer(0) as ren:
        ren.set_scene(arr, cam)
        film = ren.film(p)
        zero = film.read()

        def prime():
            film.write(zero[0], zero[1], 0)
            film.accumulate(min(a.chunk, a.spp))
            film.write(zero[0], zero[1], 0)

        def uniform(thr2):
            prime()
            chunks = 0
            t = time.perf_counter()
            while film.done < a.spp:
                film.accumulate(min(a.chunk, a.spp - film.done))
                chunks += 1
                if thr2 is not None and film.done >= 2 and film.error(thr2, want_map=False)[1]["pixels_over"] == 0:
                    break
            return (time.perf_counter() - t) * 1e3, chunks, film.done * npix

        def adaptive(thr2):
            prime()
            passes = []
            t = time.perf_counter()
            while True:
                t1 = time.perf_counter()
                fp = film.accumulate_adaptive(thr2, a.chunk).as_dict()
                ms = (time.perf_counter() - t1) * 1e3
                if fp["pixels_selected"] == 0:
                    break
                st = ren.stats()
                passes.append(dict(fp, ms=ms, idle_ms=ms - st["render_busy_ms"]))
            return (time.perf_counter() - t) * 1e3, passes

        # warm-up of both routes; the bound
        uniform(None)
        full = film.read()[0]
        thr2 = a.until * a.until if a.until is not None else film.error(0.0, want_map=False)[1]["max_e2"]
        _, chunks_u, samples_u = uniform(thr2)
        _, passes = adaptive(thr2)
        counts = film.counts()
        left = film.error(thr2, want_map=True)[0]
        # every pixel the adaptive route brought to the target holds the one-shot render's sums;
        # no pixel below the target is still over the bound
        at_target = counts == a.spp
        equal = film.read()[0][at_target].tobytes() == full[at_target].tobytes()
        over_below_target = int(((left > thr2) & ~at_target).sum())
        t_u, t_a, t_sel, per_pass = [], [], [], []
        for _ in range(a.runs):
            t_u.append(uniform(thr2)[0])
            ms, ps = adaptive(thr2)
            t_a.append(ms)
            per_pass.append(ps)
            t = time.perf_counter()
            film.accumulate_adaptive(math.inf, a.chunk)
            t_sel.append((time.perf_counter() - t) * 1e3)
        film.close()
    samples_a = sum(q["samples_added"] for q in passes)
    table = []
    for i, q in enumerate(passes):
        table.append({"pass": i, "pixels_selected": q["pixels_selected"], "samples_added": q["samples_added"],
                      "groups": q["groups"], "launches": q["launches"], "min_count": q["min_count"],
                      "max_count": q["max_count"], "ms": summary([r[i]["ms"] for r in per_pass]),
                      "ms_without_a_render_running": summary([r[i]["idle_ms"] for r in per_pass])})
    mu, ma = statistics.median(t_u), statistics.median(t_a)
    out = {
        "tool": "tools/adaptive_bench.py", "scene": a.scene, "width": a.width, "height": p.image_height,
        "target_spp": a.spp, "chunk": a.chunk, "depth": a.depth,
        "timing": "host wall clock around synchronous calls, median of alternating rounds",
        "until": math.sqrt(thr2), "threshold2": thr2,
        "uniform": {"ms": summary(t_u), "chunks": chunks_u, "samples": samples_u,
                    "ms_per_million_samples": round(mu / (samples_u / 1e6), 5)},
        "adaptive": {"ms": summary(t_a), "passes": len(passes), "samples": samples_a,
                     "ms_per_million_samples": round(ma / (samples_a / 1e6), 5),
                     "samples_over_uniform": round(samples_a / samples_u, 4), "ms_over_uniform": round(ma / mu, 4),
                     "per_sample_cost_over_uniform": round((ma / samples_a) / (mu / samples_u), 4),
                     "count_min": int(counts.min()), "count_max": int(counts.max()),
                     "count_median": float(statistics.median(counts.ravel().tolist())),
                     "pixels_at_target": int(at_target.sum()), "pixels_below_target_over_bound": over_below_target,
                     "pixels_at_target_bit_equal_to_uniform": equal, "per_pass": table},
        "select_ms": summary(t_sel),
    }
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0 if equal and over_below_target == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
