"""What the film mattes cost beside the sampled feature pass (a tool, not a test; bench.py is the
contract benchmark).  Modelled on tools/features_sampled_bench.py.

On BASELINE config 3's image (final scene, 485 spheres, thin lens, 1920x1080) with an empty film of
512 samples per pixel it times, in one process on one device after a warm-up of every shape:

  mattes_n16 / n512   ykgpu_film_mattes at n = 16 and n = 512 (device time between events,
                      yk_matte_stats.ms; the two alternate, so the table is never the cached one)
  coverage            ykgpu_film_matte_coverage of 3 ids and the sky on the n = 512 table, both
                      outputs (yk_matte_coverage_stats.ms: the kernel alone)
  features_n16        the sampled feature pass at n = 16 (yk_sampled_features_stats.ms; the pinhole
                      pass at grid 1 runs in between, so the planes are never the cached ones): the
                      yardstick, the same start and first hit per sample with the seven folds
                      instead of the table

The variants alternate round by round, so a drift of the device shows in all of them; each figure is
the median of --runs rounds, with the minimum and maximum beside it.

usage: python tools/mattes_bench.py [--runs 7] [--width 1920] [--commit ID] [--out profiles/TAG_mattes.json]
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
from uecraytracing_amd.records import (MATTE_SKY, MatteCoverageStats, MatteStats, SampledFeaturesStats,  # noqa: E402
                                       make_params)


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "runs": len(ms), "ms": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=512)
    ap.add_argument("--scene", default="final")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs must be at least 5")
    if a.spp < 16:
        ap.error("--spp must be at least 16")
    arr, cam = yk.build_scene(a.scene, 42)
    p = make_params(a.width, None, a.spp, 50, 404)
    lib = yk.load_library()
    big = a.spp
    t = {k: [] for k in ("mattes_n16", f"mattes_n{big}", "coverage", "features_n16")}
    counts = {}
    ids = np.array([0, 1, 2, MATTE_SKY], np.uint32)

    def ck(rc):
        if rc:
            raise yk.YkError(lib.ykgpu_last_error().decode())

    with yk.Renderer(0) as ren:
        ren.set_scene(arr, cam)
        film = ren.film(p)
        npix = p.row_count * p.tile_width()
        cov, grey = np.empty(npix, np.float64), np.empty(npix, np.uint8)

        def mattes(n):  # compute only: the table stays on the device
            st = MatteStats()
            ck(lib.ykgpu_film_mattes(film._f, n, None, ctypes.byref(st)))
            counts[f"mattes_n{n}"] = {k: v for k, v in st.as_dict().items() if k != "ms"}
            return st.ms

        def coverage():
            st = MatteCoverageStats()
            ck(lib.ykgpu_film_matte_coverage(film._f, ids.ctypes.data, len(ids), cov.ctypes.data, grey.ctypes.data,
                                             ctypes.byref(st)))
            counts["coverage"] = {k: v for k, v in st.as_dict().items() if k != "ms"}
            return st.ms

        def features(n):
            ms = ctypes.c_double(0.0)
            ck(lib.ykgpu_film_features(film._f, 1, None, None, ctypes.byref(ms)))  # (replaces the sampled planes)
            st = SampledFeaturesStats()
            ck(lib.ykgpu_film_features_sampled(film._f, n, None, None, ctypes.byref(st)))
            counts[f"features_n{n}"] = {"samples": st.samples, "hits": st.hits, "redo_pixels": st.redo_pixels}
            return st.ms

        mattes(16), features(16), mattes(big), coverage()  # warm-up: every shape once
        for _ in range(a.runs):
            t["mattes_n16"].append(mattes(16))
            t["features_n16"].append(features(16))
            t[f"mattes_n{big}"].append(mattes(big))
            t["coverage"].append(coverage())
        film.close()
    assert min(min(v) for v in t.values()) > 0.0  # (no figure is a cached pass's)
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {
        "tool": "tools/mattes_bench.py", "commit": a.commit, "scene": a.scene, "width": a.width, "height": p.image_height,
        "film_target_spp": a.spp, "spheres": len(arr), "lens_radius": cam.lens_radius, "pass_counts": counts,
        "timing": "device time between events on the stream; medians of alternating rounds",
        "calls": {k: summary(v) for k, v in t.items()},
        "mattes_n16_over_features_n16": round(med["mattes_n16"] / med["features_n16"], 4),
        f"mattes_n{big}_per_16_samples_over_features_n16": round(med[f"mattes_n{big}"] * 16 / big / med["features_n16"], 4),
        "table_bytes": npix * 80,
    }
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
