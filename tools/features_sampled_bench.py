"""What the sampled feature pass costs beside the pinhole pass and the render (a tool, not a test;
bench.py is the contract benchmark).  Modelled on tools/features_bench.py.

On BASELINE config 3's image (final scene, thin lens, 1920x1080, depth 50) with a film of 64 samples
per pixel it times, in one process on one device after a warm-up of every shape:

  chunk_16spp       one ykgpu_film_accumulate(16) into the emptied film (host wall clock): the render
                    of as many samples as the largest pass below looks at
  sampled_n4/n16    the sampled feature pass at n = 4 and n = 16 (device time between events,
                    yk_sampled_features_stats.ms; each round runs the pinhole pass in between, so the
                    pass is never the cached one)
  pinhole_g2        the pinhole pass at grid 2 (ykgpu_film_features' ms), never cached either
  guided_sampled    the whole ykgpu_film_denoise_guided_sampled call at the defaults, RGB8 only, the
                    planes not cached: features_ms + moments_ms + filter_ms on the device, and the
                    call's host wall clock

The variants alternate round by round, so a drift of the device shows in all of them; each figure is
the median of --runs rounds, with the minimum and maximum beside it.

usage: python tools/features_sampled_bench.py [--runs 7] [--width 1920] [--commit ID]
       [--out profiles/TAG_features_sampled.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uecraytracing_amd as yk  # noqa: E402
from uecraytracing_amd.records import SampledFeaturesStats, make_params  # noqa: E402

CHUNK = 16


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "runs": len(ms), "ms": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--scene", default="final")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs must be at least 5")
    arr, cam = yk.build_scene(a.scene, 42)
    p = make_params(a.width, None, a.spp, a.depth, 404)
    dp, fp, n_default = yk.guided_sampled_defaults()
    lib = yk.load_library()
    t = {k: [] for k in ("chunk_16spp", "sampled_n4", "sampled_n16", "pinhole_g2", "guided_sampled_device",
                         "guided_sampled_wall", "guided_sampled_features", "guided_sampled_moments",
                         "guided_sampled_filter")}
    counts = {}
    with yk.Renderer(0) as ren:
        ren.set_scene(arr, cam)
        film = ren.film(p)
        zero = film.read()

        def chunk():
            film.write(zero[0], zero[1], 0)
            t0 = time.perf_counter()
            film.accumulate(CHUNK)
            return (time.perf_counter() - t0) * 1e3

        def pinhole():  # compute and cache only: no copy in the figure
            ms = ctypes.c_double(0.0)
            if lib.ykgpu_film_features(film._f, 2, None, None, ctypes.byref(ms)):
                raise yk.YkError(lib.ykgpu_last_error().decode())
            return ms.value

        def sampled(n):
            st = SampledFeaturesStats()
            if lib.ykgpu_film_features_sampled(film._f, n, None, None, ctypes.byref(st)):
                raise yk.YkError(lib.ykgpu_last_error().decode())
            counts[n] = {"samples": st.samples, "hits": st.hits, "redo_pixels": st.redo_pixels}
            return st.ms

        def guided():
            t0 = time.perf_counter()
            _, _, st = film.denoise_guided_sampled(dp, fp, n_default, want_mean=False)
            return (time.perf_counter() - t0) * 1e3, st

        chunk()  # warm-up: every shape once
        sampled(4), pinhole(), sampled(16), pinhole(), guided()
        for _ in range(a.runs):
            t["chunk_16spp"].append(chunk())
            t["sampled_n4"].append(sampled(4))
            t["pinhole_g2"].append(pinhole())
            t["sampled_n16"].append(sampled(16))
            pinhole()  # (the planes are the pinhole pass's again: the guided call computes its own)
            wall, st = guided()
            assert st["features_ms"] > 0.0
            t["guided_sampled_wall"].append(wall)
            t["guided_sampled_device"].append(st["features_ms"] + st["moments_ms"] + st["filter_ms"])
            t["guided_sampled_features"].append(st["features_ms"])
            t["guided_sampled_moments"].append(st["moments_ms"])
            t["guided_sampled_filter"].append(st["filter_ms"])
        film.close()
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {
        "tool": "tools/features_sampled_bench.py", "commit": a.commit, "scene": a.scene, "width": a.width, "height": p.image_height,
        "film_target_spp": a.spp, "depth": a.depth, "spheres": len(arr), "lens_radius": cam.lens_radius,
        "colour": dp.as_dict(), "features": fp.as_dict(), "n_default": n_default, "pass_counts": counts,
        "timing": "chunk and *_wall: host wall clock around synchronous calls; sampled_*, pinhole_* and *_device: between "
                  "events on the stream; medians of alternating rounds",
        "calls": {k: summary(v) for k, v in t.items()},
        "sampled_n16_over_chunk_16spp": round(med["sampled_n16"] / med["chunk_16spp"], 4),
        "sampled_n16_over_pinhole_g2": round(med["sampled_n16"] / med["pinhole_g2"], 4),
        "sampled_n4_over_pinhole_g2": round(med["sampled_n4"] / med["pinhole_g2"], 4),
    }
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
