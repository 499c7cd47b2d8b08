"""The GPU side of tests/test_gpu_mattes_fallbacks.py (TEST INFRASTRUCTURE ONLY), run in a fresh
process per library: `mattes_child.py <dir>` loads the library YKGPU_LIB_OVERRIDE names (the product's
without it), runs the film mattes of the 485-sphere final scene on cuda:0 and leaves the table in
<dir>/out.npz and the statistics in <dir>/stats.json.  It compares nothing: the test does."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main():
    folder = sys.argv[1]
    import uecraytracing_amd as yk
    from uecraytracing_amd.records import make_params
    arr, cam = yk.read_scene(os.path.join(yk.SCENE_DIR, "final_seed42.yks"))
    with yk.Renderer(0) as ren:
        ren.set_scene(arr, cam)
        with ren.film(make_params(32, 18, 8, 50, 404)) as film:
            table, stats = film.mattes(8)
            cov, grey, cstats = film.matte_coverage([int(table["id"][9, 16, 0]), 0])
    np.savez(os.path.join(folder, "out.npz"), table=table, cov=cov, grey=grey)
    with open(os.path.join(folder, "stats.json"), "w") as f:
        json.dump(dict(mattes=stats, coverage=cstats), f)


if __name__ == "__main__":
    main()
