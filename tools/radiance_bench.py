"""What a batch of radiance queries costs (a tool, not a test; bench.py is the contract benchmark).
Modelled on tools/cast_bench.py.

On the final scene (seed 42), in one process on one device after a warm-up of every shape:

  (a) camera     the camera start rays of every sample of 1920x1080x8 (yk_camera_sample_rays) through
                 ykgpu_radiance_rays: yk_radiance_stats.kernel_ms (device time between events, the
                 chunks' sum) and the share of it in the starts kernel.  The yardstick is the render
                 itself on the same samples: one synced ykgpu_render_sums of that image
                 (yk_render_stats.kernel_ms), whose per-pixel sums the folded query must equal.
  (b) scan       YK_RADIANCE_LINEAR_SCAN on every 15th ray of (a) (2^20 at most), beside the tree on the same rays.
  (c) incoherent the second-segment rays of a 1920x1080x1 ykgpu_render_trace (every sample whose path
                 scattered once), with seeds of their own.
  (d) xor128     set (a)'s image with the other engine (no starts kernel).

The variants alternate round by round, so a drift of the device shows in all of them; each figure is
the median of --runs rounds with the minimum and maximum beside it.  Segments and words per ray come
from one YK_RADIANCE_COUNT_WORK query per set.

usage: python tools/radiance_bench.py [--runs 7] [--width 1920] [--spp 8] [--commit ID] [--out profiles/TAG_radiance.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uecraytracing_amd as yk  # noqa: E402
from uecraytracing_amd import records  # noqa: E402
from uecraytracing_amd.records import make_params  # noqa: E402


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "runs": len(ms), "ms": [round(x, 4) for x in ms]}


def image_rays(cam, p):
    ys, xs, ss = np.meshgrid(np.arange(p.image_height, dtype=np.uint32), np.arange(p.image_width, dtype=np.uint32),
                             np.arange(p.samples_per_pixel, dtype=np.uint32), indexing="ij")
    return yk.camera_sample_rays(cam, p, ys, xs, ss)


def fold(colours, p):
    c = colours.reshape(p.image_height, p.image_width, p.samples_per_pixel, 3)
    acc = np.zeros((p.image_height, p.image_width, 3), np.float64)
    for s in range(p.samples_per_pixel):
        acc = acc + c[:, :, s]
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--scene", default="final")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs must be at least 5")
    arr, cam = yk.build_scene(a.scene, 42)
    p = make_params(a.width, None, a.spp, 50, 404)
    px = make_params(a.width, None, a.spp, 50, 404, rng=records.RNG_XOR128)
    W, H = p.image_width, p.image_height
    keys = ("render_sums", "camera", "camera_starts", "render_sums_x128", "camera_x128", "sub_tree", "sub_scan", "incoherent")
    t = {k: [] for k in keys}
    with yk.Renderer(0) as ren:
        ren.set_scene(arr, cam)
        rays, rays_x = image_rays(cam, p), image_rays(cam, px)
        sub = np.ascontiguousarray(rays[:: max(1, len(rays) >> 20)][: 1 << 20])
        trace, counts = ren.render_trace(make_params(a.width, None, 1, 50, 404), 2)
        second = counts.reshape(-1) >= 2
        seg = trace.reshape(-1, 2, 6)[second, 1]
        inc = np.zeros(len(seg), records.PATH_RAY_DTYPE)
        inc["origin"], inc["direction"] = seg[:, 0:3], seg[:, 3:6]
        inc["seed"] = np.arange(len(seg), dtype=np.uint32)
        del trace, seg

        def query(r, par, **kw):
            out = ren.radiance_rays(r, par.max_depth, par.t_min, par.rng, **kw)
            return ren.radiance_stats(), out

        def render(par):
            sums = ren.render_sums(par)
            return ren.stats(), sums

        # warm-up: every shape once, and the query folded against the render
        st, sums = render(p)
        sclk = st["sclk_mhz"]
        _, out = query(rays, p)
        equal = fold(out["colour"], p).tobytes() == sums.tobytes()
        _, sums_x = render(px)
        _, out_x = query(rays_x, px)
        equal_x = fold(out_x["colour"], px).tobytes() == sums_x.tobytes()
        del out, out_x, sums, sums_x
        query(sub, p), query(sub, p, linear_scan=True), query(inc, p)
        for _ in range(a.runs):
            t["render_sums"].append(render(p)[0]["kernel_ms"])
            st = query(rays, p)[0]
            t["camera"].append(st["kernel_ms"])
            t["camera_starts"].append(st["starts_ms"])
            t["render_sums_x128"].append(render(px)[0]["kernel_ms"])
            t["camera_x128"].append(query(rays_x, px)[0]["kernel_ms"])
            t["sub_tree"].append(query(sub, p)[0]["kernel_ms"])
            t["sub_scan"].append(query(sub, p, linear_scan=True)[0]["kernel_ms"])
            t["incoherent"].append(query(inc, p)[0]["kernel_ms"])
        work = {}
        for name, r in (("camera", rays), ("incoherent", inc)):
            st, out = query(r, p, count_work=True)
            work[name] = {"rays": st["rays"], "segments_per_ray": round(st["segments"] / st["rays"], 3),
                          "words_per_ray": round(st["words"] / st["rays"], 2), "mt_fallbacks": st["mt_fallbacks"],
                          "scan_segments": st["scan_segments"], "out_of_domain": st["out_of_domain"], "lanes": st["lanes"],
                          "max_segments": int(out["segments"].max())}
            del out
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {
        "tool": "tools/radiance_bench.py", "commit": a.commit, "scene": a.scene, "spheres": len(arr), "width": W, "height": H,
        "spp": a.spp, "sclk_mhz": round(sclk, 1),
        "timing": "device time between events on the context's stream (yk_radiance_stats.kernel_ms, "
                  "yk_render_stats.kernel_ms of a synced ykgpu_render_sums); medians of alternating rounds",
        "query_equals_render_sums": {"mt19937": equal, "xor128": equal_x},
        "calls": {k: summary(v) for k, v in t.items()},
        "work": work,
        "mrays_per_s": {"camera": round(len(rays) / med["camera"] / 1e3, 1),
                        "camera_x128": round(len(rays_x) / med["camera_x128"] / 1e3, 1),
                        "render_sums": round(len(rays) / med["render_sums"] / 1e3, 1),
                        "render_sums_x128": round(len(rays) / med["render_sums_x128"] / 1e3, 1),
                        "sub_tree": round(len(sub) / med["sub_tree"] / 1e3, 1),
                        "sub_scan": round(len(sub) / med["sub_scan"] / 1e3, 1),
                        "incoherent": round(len(inc) / med["incoherent"] / 1e3, 1)},
        "starts_share": round(med["camera_starts"] / med["camera"], 4),
        "query_over_render": {"mt19937": round(med["camera"] / med["render_sums"], 3),
                              "xor128": round(med["camera_x128"] / med["render_sums_x128"], 3)},
    }
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
