"""The workloads beside the contract bench for one library (YKGPU_LIB_OVERRIDE names another build of
libykgpu.so, else the tree's): the median of 40 ykgpu_set_scene calls, the first frame call, synced
calls of the frame, frames with a new seed0 each (the seed table's fill calls), the xor128 frame, rank 0's
tile of the 8-way split, the FP32 frame, config 5 and a frame without sky
(tests/golden/room5.yks at 64 spp).  One JSON line; run it once per library, alternating, to compare
two builds (profiles/r18_sky_blocks/other_workloads_ab.json).  AB_ONLY=tile stops after the tile.
usage: python tools/other_workloads_ab.py <tag>"""
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401
import uecraytracing_amd as yk  # noqa: E402
from uecraytracing_amd.records import PRECISION_FP32, RNG_XOR128, make_params  # noqa: E402
from uecraytracing_amd.tiles import rank_tile  # noqa: E402

out = {"tag": sys.argv[1], "lib": os.environ.get("YKGPU_LIB_OVERRIDE", "tree")}
W, H = 1920, 1080
final = yk.read_scene(os.path.join(yk.SCENE_DIR, "final_seed42.yks"))
glass = yk.read_scene(os.path.join(yk.SCENE_DIR, "glass_seed42.yks"))
room = yk.read_scene(os.path.join(ROOT, "tests", "golden", "room5.yks"))


def timed(ren, p, n):
    ts, img = [], None
    for _ in range(n):
        t = time.perf_counter()
        img = ren.render(p)
        ts.append((time.perf_counter() - t) * 1e3)
    return {"ms": [round(t, 3) for t in ts], "sha": hashlib.sha256(img.tobytes()).hexdigest()[:16]}


with yk.Renderer(0) as ren:
    ts = []
    for _ in range(40):
        t = time.perf_counter()
        ren.set_scene(*final)
        ts.append((time.perf_counter() - t) * 1e3)
    out["set_scene_ms_median_of_40"] = round(statistics.median(ts), 4)
    p = make_params(W, H, 512, 50, 404)
    t = time.perf_counter()
    ren.render(p)
    out["first_call_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    # one-shot use: a new view, then one frame — ykgpu_set_scene with the camera moved a little
    # further each time, then one synced 512-spp frame; wall ms of each pair
    ts = []
    for k in range(8):
        cam = type(final[1]).from_buffer_copy(final[1])
        cam.origin[1] += 0.01 * (k + 1)
        t = time.perf_counter()
        ren.set_scene(final[0], cam)
        ren.render(p)
        ts.append(round((time.perf_counter() - t) * 1e3, 3))
    out["set_scene_plus_one_frame_ms"] = ts
    ren.set_scene(*final)
    ren.render(p)
    out["synced_frame"] = timed(ren, p, 3)
    st = ren.stats()
    out["frame_stats"] = {k: st[k] for k in ("launches", "launch_spp", "device_bytes", "call_bytes", "kernel_ms",
                                             "warmup_ms", "resolve_ms", "render_busy_ms")}
    # seed0 changed on every call: with the seed table every such call fills it and none reads it
    ts = []
    for k in range(6):
        t = time.perf_counter()
        ren.render(make_params(W, H, 512, 50, 1000 + k))
        ts.append(round((time.perf_counter() - t) * 1e3, 3))
    out["new_seed0_every_call_ms"] = ts
    ren.render(p)
    # the walk-free engine on the same build: the floor under any saving on the walks
    out["xor128_frame"] = timed(ren, make_params(W, H, 512, 50, 404, rng=RNG_XOR128), 3)
    ren.render(p)
    out["tile_rank0_of_8"] = timed(ren, make_params(W, H, 512, 50, 404, **rank_tile(0, 8, H, W, "rows")), 6)
    if os.environ.get("AB_ONLY") == "tile":
        print(json.dumps(out), flush=True)
        sys.exit(0)
    out["fp32_frame"] = timed(ren, make_params(W, H, 512, 50, 404, precision=PRECISION_FP32), 3)
    ren.set_scene(*glass)
    out["config5_glass_4096spp_d200"] = timed(ren, make_params(W, H, 4096, 200, 404), 2)
    ren.set_scene(*room)
    out["no_sky_room5_64spp"] = timed(ren, make_params(W, H, 64, 50, 404), 5)
    out["no_sky_stats"] = {k: ren.stats()[k] for k in ("launches", "launch_spp", "device_bytes")}
print(json.dumps(out), flush=True)
