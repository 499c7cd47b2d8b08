"""What a batch of ray queries costs (a tool, not a test; bench.py is the contract benchmark).
Modelled on tools/features_bench.py.

On the final scene (seed 42), in one process on one device after a warm-up of every shape:

  (a) coherent   the 2,073,600 pixel-centre pinhole rays of 1920x1080 through ykgpu_cast_rays:
                 yk_cast_stats.kernel_ms (device time between events, the chunks' sum), closest and
                 any-hit.  The yardstick is ykgpu_film_features(grid = 1) on the same tile — the same
                 rays through the feature kernel's 485-sphere ordered scan (its device time; each round
                 asks for grid 2 first, so the pass is never the cached one).
  (b) incoherent the second-segment rays of a 1920x1080x1 ykgpu_render_trace (every sample whose
                 path scattered once): Mrays/s of closest and any-hit from kernel_ms, and node visits
                 and sphere tests per ray from a YK_CAST_COUNT_WORK cast.
  (c) scan       YK_CAST_LINEAR_SCAN on set (a).

The variants alternate round by round, so a drift of the device shows in all of them; each figure is
the median of --runs rounds with the minimum and maximum beside it.

usage: python tools/cast_bench.py [--runs 7] [--width 1920] [--commit ID] [--out profiles/TAG_cast.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uecraytracing_amd as yk  # noqa: E402
from uecraytracing_amd.records import make_params  # noqa: E402

INF = float("inf")


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "runs": len(ms), "ms": [round(x, 4) for x in ms]}


def pixel_rays(cam, W, H):
    """The feature pass's a = b = 0.5 sub-ray of every pixel (include/ykgpu.h "film features")."""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u = (xs + 0.5) / np.float64(W)
    v = (((np.float64(H) - ys) - 1.0) + 0.5) / np.float64(H)
    o = np.array(tuple(cam.origin))
    d = np.stack([((cam.lower_left_corner[k] + cam.horizontal[k] * u) + cam.vertical[k] * v) - o[k] for k in range(3)], -1)
    d = d.reshape(-1, 3)
    return np.broadcast_to(o, d.shape).copy(), d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--scene", default="final")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs must be at least 5")
    arr, cam = yk.build_scene(a.scene, 42)
    p = make_params(a.width, None, 1, 50, 404)
    W, H = p.image_width, p.image_height
    lib = yk.load_library()
    keys = ("features_g1", "coherent_closest", "coherent_any", "coherent_scan", "incoherent_closest", "incoherent_any")
    t = {k: [] for k in keys}
    with yk.Renderer(0) as ren:
        ren.set_scene(arr, cam)
        co, cd = pixel_rays(cam, W, H)
        rays, counts = ren.render_trace(p, 2)
        sclk = ren.stats()["sclk_mhz"]
        second = counts.reshape(-1) >= 2
        seg = rays.reshape(-1, 2, 6)[second, 1]
        io, idr = np.ascontiguousarray(seg[:, 0:3]), np.ascontiguousarray(seg[:, 3:6])
        del rays
        film = ren.film(p)

        def features(grid):  # compute and cache only: no copy in the figure
            ms = ctypes.c_double(0.0)
            if lib.ykgpu_film_features(film._f, grid, None, None, ctypes.byref(ms)):
                raise yk.YkError(lib.ykgpu_last_error().decode())
            return ms.value

        def cast(o, d, **kw):
            hits = ren.cast_rays(o, d, 0.001, INF, **kw)
            return ren.cast_stats(), hits

        features(2), features(1)  # warm-up: every shape once
        for kw in ({}, {"any_hit": True}, {"linear_scan": True}):
            cast(co, cd, **kw)
        cast(io, idr), cast(io, idr, any_hit=True)
        for _ in range(a.runs):
            features(2)
            t["features_g1"].append(features(1))
            t["coherent_closest"].append(cast(co, cd)[0]["kernel_ms"])
            t["coherent_any"].append(cast(co, cd, any_hit=True)[0]["kernel_ms"])
            t["coherent_scan"].append(cast(co, cd, linear_scan=True)[0]["kernel_ms"])
            t["incoherent_closest"].append(cast(io, idr)[0]["kernel_ms"])
            t["incoherent_any"].append(cast(io, idr, any_hit=True)[0]["kernel_ms"])
        work = {}
        for name, (o, d) in (("coherent", (co, cd)), ("incoherent", (io, idr))):
            st, hits = cast(o, d, count_work=True)
            work[name] = {"rays": st["rays"], "hit_share": round(st["hits"] / st["rays"], 4), "scan_rays": st["scan_rays"],
                          "node_visits_per_ray": round(st["node_visits"] / st["rays"], 3),
                          "sphere_tests_per_ray": round(st["sphere_tests"] / st["rays"], 3)}
        film.close()
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {
        "tool": "tools/cast_bench.py", "commit": a.commit, "scene": a.scene, "spheres": len(arr), "width": W, "height": H,
        "sclk_mhz": round(sclk, 1),
        "timing": "device time between events on the context's stream (yk_cast_stats.kernel_ms, ykgpu_film_features' "
                  "ms); medians of alternating rounds",
        "calls": {k: summary(v) for k, v in t.items()},
        "work": work,
        "coherent_cast_over_features_g1": round(med["coherent_closest"] / med["features_g1"], 4),
        "coherent_mrays_per_s": {k: round(len(co) / med["coherent_" + k] / 1e3, 1) for k in ("closest", "any", "scan")},
        "incoherent_mrays_per_s": {k: round(len(io) / med["incoherent_" + k] / 1e3, 1) for k in ("closest", "any")},
    }
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
