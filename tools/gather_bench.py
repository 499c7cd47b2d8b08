"""What a batch of gather queries costs, beside the composed route it replaces (a tool, not a test;
bench.py is the contract benchmark).  Modelled on tools/radiance_bench.py.

On the final scene (seed 42), in one process on one device: the points are the first hits of the
1920x1080 pixel-centre pinhole rays (ykgpu_cast_rays), each with a seed of its own.  Per engine
(mt19937, xor128) and N in {4, 64}, after a warm-up of every shape in which the two routes' records
are compared as bytes:

  gather    ykgpu_gather_points on the points: yk_gather_stats.kernel_ms (device time between
            events, the chunks' sum), its parts in the starts and the fold kernel, and total_ms, the
            call's host wall clock;
  composed  the same records the way a caller had to make them before: yk_gather_sample_rays on the
            host, ykgpu_radiance_rays (yk_radiance_stats.kernel_ms and total_ms), the numpy fold;
            the three parts' host wall clocks and their sum.

At N = 64 the composed route would stage 14 GB of rays and records for the whole image, so both
routes run on every --stride64-th point there ("compared"), and the gather alone also runs on all
points ("all").  The variants alternate round by round; each figure is the median of --runs rounds
with the minimum and maximum beside it.

usage: python tools/gather_bench.py [--runs 7] [--width 1920] [--commit ID] [--out profiles/TAG_gather.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uecraytracing_amd as yk  # noqa: E402
from uecraytracing_amd import records  # noqa: E402

SKY, OOD, FALLBACK = records.RAD_SKY, records.RAD_OUT_OF_DOMAIN, records.RAD_MT_FALLBACK


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "runs": len(ms)}


def pixel_rays(cam, W, H):
    """the pixel-centre pinhole rays (include/ykgpu.h "film features": the sub-ray with a = b = 0.5)"""
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    u = ((xs + 0.5) / W).reshape(-1, 1)
    v = ((H - ys - 1 + 0.5) / H).reshape(-1, 1)
    o = np.array(tuple(cam.origin), np.float64)
    d = ((np.array(tuple(cam.lower_left_corner)) + np.array(tuple(cam.horizontal)) * u) + np.array(tuple(cam.vertical)) * v) - o
    return np.broadcast_to(o, d.shape).copy(), d


def fold(recs):
    """records.GATHER_DTYPE[N] from records.RADIANCE_DTYPE[N, n]: include/ykgpu.h "gather queries" """
    n, ns = recs.shape
    out = np.zeros(n, records.GATHER_DTYPE)
    s, q = np.zeros((n, 3)), np.zeros((n, 3))
    for k in range(ns):
        c = recs["colour"][:, k, :]
        s = s + c
        q = q + c * c
    out["sum"], out["sumsq"], out["samples"] = s, q, ns
    out["open"] = (((recs["flags"] & SKY) != 0) & (recs["segments"] == 1)).sum(1)
    out["flags"] = np.bitwise_or.reduce(recs["flags"] & (OOD | FALLBACK), axis=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--stride64", type=int, default=64, help="the composed route at N = 64 runs on every stride64-th point")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs must be at least 5")
    arr, cam = yk.build_scene("final", 42)
    W, H = a.width, records.image_height_for(a.width)
    cases = [(rng, name, n) for n in (4, 64) for rng, name in ((records.RNG_MT19937, "mt19937"), (records.RNG_XOR128, "xor128"))]
    result = {}
    with yk.Renderer(0) as ren:
        ren.set_scene(arr, cam)
        o, d = pixel_rays(cam, W, H)
        hits = ren.cast_rays(o, d)
        hits = hits[(hits["flags"] & records.HIT_HIT) != 0]
        del o, d
        points = yk.gather_points(hits["p"], hits["normal"], (np.arange(len(hits), dtype=np.uint64) * 2654435761 % 2 ** 32).astype(np.uint32))
        sets = {4: points, 64: np.ascontiguousarray(points[:: a.stride64])}

        def gather(pts, n, rng):
            ren.gather_points(pts, n, 50, records.T_MIN, rng)
            return ren.gather_stats()

        def composed(pts, n, rng):
            t0 = time.perf_counter()
            rays = yk.gather_sample_rays(pts, n, rng)
            t1 = time.perf_counter()
            recs = ren.radiance_rays(rays.reshape(-1), 50, records.T_MIN, rng)
            st = ren.radiance_stats()
            t2 = time.perf_counter()
            out = fold(recs.reshape(rays.shape))
            t3 = time.perf_counter()
            return out, st, (1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2))

        t = {}
        for rng, name, n in cases:  # warm-up of every shape; the two routes' records as bytes
            key = f"{name}_n{n}"
            got = ren.gather_points(sets[n], n, 50, records.T_MIN, rng)
            want, _, _ = composed(sets[n], n, rng)
            st = ren.gather_stats()
            result[key] = {"engine": name, "n_samples": n, "points_compared": len(sets[n]), "rays_compared": len(sets[n]) * n,
                           "gather_equals_composed": got.tobytes() == want.tobytes(),
                           "open_share": round(st["open"] / st["rays"], 4), "points_out_of_domain": st["out_of_domain"],
                           "points_mt_fallback": st["mt_fallbacks"]}
            t[key] = {k: [] for k in ("gather_kernel", "gather_starts", "gather_fold", "gather_wall", "query_kernel", "query_starts",
                                      "query_wall", "host_rays", "host_fold", "composed_wall", "gather_all_kernel", "gather_all_wall")}
            del got, want
            if n == 64:
                gather(points, n, rng)
        for _ in range(a.runs):
            for rng, name, n in cases:
                k = t[f"{name}_n{n}"]
                st = gather(sets[n], n, rng)
                k["gather_kernel"].append(st["kernel_ms"]), k["gather_starts"].append(st["starts_ms"])
                k["gather_fold"].append(st["fold_ms"]), k["gather_wall"].append(st["total_ms"])
                _, qs, (h0, h1, h2) = composed(sets[n], n, rng)
                k["query_kernel"].append(qs["kernel_ms"]), k["query_starts"].append(qs["starts_ms"]), k["query_wall"].append(qs["total_ms"])
                k["host_rays"].append(h0), k["host_fold"].append(h2), k["composed_wall"].append(h0 + h1 + h2)
                if n == 64:
                    st = gather(points, n, rng)
                    k["gather_all_kernel"].append(st["kernel_ms"]), k["gather_all_wall"].append(st["total_ms"])
        ren.render_sums(records.make_params(256, None, 8, 50, 404))  # (a render's statistics carry the shader clock)
        sclk = ren.stats()["sclk_mhz"]
    for key, k in t.items():
        r = result[key]
        rays = r["rays_compared"]
        r["calls"] = {name: summary(v) for name, v in k.items() if v}
        med = {name: statistics.median(v) for name, v in k.items() if v}
        r["mrays_per_s"] = {"gather": round(rays / med["gather_kernel"] / 1e3, 1), "query": round(rays / med["query_kernel"] / 1e3, 1)}
        if "gather_all_kernel" in med:
            r["points_all"] = len(points)
            r["mrays_per_s"]["gather_all"] = round(len(points) * r["n_samples"] / med["gather_all_kernel"] / 1e3, 1)
        r["gather_over_query_device"] = round(med["gather_kernel"] / med["query_kernel"], 4)
        r["query_spread"] = round((max(k["query_kernel"]) - min(k["query_kernel"])) / med["query_kernel"], 4)
        r["composed_over_gather_wall"] = round(med["composed_wall"] / med["gather_wall"], 2)
    out = {"tool": "tools/gather_bench.py", "commit": a.commit, "scene": "final", "scene_seed": 42, "spheres": len(arr),
           "width": W, "height": H, "points": len(points), "sclk_mhz": round(sclk, 1),
           "timing": "device: time between events on the context's stream (yk_gather_stats / yk_radiance_stats kernel_ms); "
                     "wall: the call's host clock (total_ms) and time.perf_counter around the host steps; medians of "
                     "alternating rounds",
           "cases": result}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
