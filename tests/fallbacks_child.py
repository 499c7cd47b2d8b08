"""The GPU side of tests/test_gpu_fallbacks.py (TEST INFRASTRUCTURE ONLY), run in a fresh process per
library: `fallbacks_child.py sky|query <dir>` loads the library YKGPU_LIB_OVERRIDE names (the product's
without it), runs the group's calls on cuda:0 and leaves every result in <dir>/out.npz and the
statistics in <dir>/stats.json.  It compares nothing: the test does, against the CPU references and
against the other library's files."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

RENDER_KEYS = ("launches", "launch_spp", "samples", "mt_fallbacks", "kernel_ms", "warmup_ms")


def render_stats(ren):
    st = ren.stats()
    return {k: st[k] for k in RENDER_KEYS}


def sky(out, stats):
    """The calls of test_gpu_sky_blocks.py that reach yk_sky_samples, on its scenes."""
    import torch

    import test_gpu_sky_blocks as sky_cases
    import uecraytracing_amd as yk
    from uecraytracing_amd import tiles
    from uecraytracing_amd.records import make_params
    W, H, SPP, DEPTH = sky_cases.W, sky_cases.H, sky_cases.SPP, sky_cases.DEPTH

    def call(ren, key, p):
        out[key + "_rgb"] = ren.render(p)
        stats[key] = render_stats(ren)
        out[key + "_sums"] = ren.render_sums(p)

    with yk.Renderer(0) as ren:
        ren.set_scene(*sky_cases.scene("pitched", 0.05))
        call(ren, "whole", make_params(W, H, SPP, DEPTH, 404))
        for rank in (0, 1):
            call(ren, f"rows{rank}", make_params(W, H, SPP, DEPTH, 404, rows=tiles.tile_rows(rank, 2, H)))
            call(ren, f"cols{rank}", make_params(W, H, SPP, DEPTH, 404, cols=tiles.tile_cols(rank, 2, W)))
        for spp in (1, 5):
            call(ren, f"spp{spp}", make_params(W, H, spp, DEPTH, 404))
        # three calls enqueued without a wait between them, then a synced one
        p = make_params(W, H, SPP, DEPTH, 404)
        outs = [torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0") for _ in range(3)]
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        for o in outs:
            ren.render_async(p, o.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        for k, o in enumerate(outs):
            out[f"async{k}_rgb"] = o.cpu().numpy()
        out["async_synced_rgb"] = ren.render(p)
        # the sky-only call, and a path call right after it on the same context
        ren.set_scene(*sky_cases.scene("all_sky", 0.05))
        call(ren, "all_sky", p)
        ren.set_scene(*sky_cases.scene("no_sky", 0.05))
        call(ren, "no_sky", p)
        # the control: no lens, so no lens loop and nothing listed
        ren.set_scene(*sky_cases.scene("pitched", 0.0))
        call(ren, "lens0", p)


def query(out, stats, inputs):
    """The four query kernels on the 485-sphere final scene, and casts of a one-leaf and a one-node tree."""
    import uecraytracing_amd as yk
    from uecraytracing_amd import records
    from uecraytracing_amd.records import make_params
    arr, cam = yk.read_scene(os.path.join(yk.SCENE_DIR, "final_seed42.yks"))
    with yk.Renderer(0) as ren:
        ren.set_scene(arr, cam)
        # the path kernel's own traced rays (the render kernels are the product's in every library)
        cap = 16
        rays, counts = ren.render_trace(make_params(16, 9, 4, 50, 404), cap)
        rays, counts = rays.reshape(-1, cap, 6), np.minimum(counts.reshape(-1), cap)
        flat = np.ascontiguousarray(rays[np.arange(cap)[None, :] < counts[:, None]])
        out["traced"] = flat
        o = np.concatenate([inputs["pixel_o"], flat[:, 0:3]])
        d = np.concatenate([inputs["pixel_d"], flat[:, 3:6]])
        for mode in ("closest", "any"):
            out["cast_" + mode] = ren.cast_rays(o, d, any_hit=mode == "any")
            stats["cast_" + mode] = ren.cast_stats()
        for name, rng in (("mt", records.RNG_MT19937), ("x128", records.RNG_XOR128)):
            for size in ("small", "big"):
                key = f"rad_{size}_{name}"
                out[key] = ren.radiance_rays(inputs[key], 50, records.T_MIN, rng, count_work=True)
                stats[key] = ren.radiance_stats()
        out["gather64"] = ren.gather_points(inputs["points"][:64], 16)
        stats["gather64"] = ren.gather_stats()
        out["gather8"] = ren.gather_points(inputs["points"][:8], 4)
        with ren.film(make_params(32, 18, 8, 50, 404)) as film:
            out["feat_mean"], out["feat_var"], stats["feat"] = film.features_sampled(8)
        # one sphere: the tree's root is a leaf code; two: one node over two leaves
        import refscenes
        for n in (1, 2):
            ren.set_scene(refscenes.ref4()[:n], refscenes.reference_camera())
            for mode in ("closest", "any"):
                key = f"leaf{n}_{mode}"
                out[key] = ren.cast_rays(inputs["leaf_o"], inputs["leaf_d"], any_hit=mode == "any", count_work=True)
                stats[key] = ren.cast_stats()


def main():
    group, folder = sys.argv[1], sys.argv[2]
    out, stats = {}, {}
    if group == "sky":
        sky(out, stats)
    else:
        query(out, stats, np.load(os.path.join(folder, "inputs.npz")))
    np.savez(os.path.join(folder, "out.npz"), **out)
    with open(os.path.join(folder, "stats.json"), "w") as f:
        json.dump(stats, f)


if __name__ == "__main__":
    main()
