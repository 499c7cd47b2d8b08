"""The GPU side of tests/test_gpu_seed_table.py's child-process cases (TEST INFRASTRUCTURE ONLY):
`seed_table_child.py <dir>` runs the product library in a fresh process, under whatever
YKGPU_SEED_TABLE / YKGPU_SEED_TABLE_MAX_MB the parent set; SEED_TABLE_CHILD_POISON=1 first
calls the test hook yk_seed_table_test(0x80000000): every fill then stores x_397 with its top bit
flipped.  For each of the
test's scenes it runs, on a context of its own: the first call of a key (it walks), the second (it fills),
two more (sums, then image: they read), then the same with seed0 + 1 (image, fill, sums).  It leaves the images and sums in <dir>/out.npz and each call's device_bytes in
<dir>/stats.json.  It compares nothing: the test does."""
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
    import test_gpu_seed_table as cases
    import uecraytracing_amd as yk
    out, stats = {}, {}
    if os.environ.get("SEED_TABLE_CHILD_POISON"):
        yk.load_library().yk_seed_table_test(0x80000000)
    for name, lens in cases.CASES:
        key = f"{name}-{lens}"
        with yk.Renderer(0) as ren:
            ren.set_scene(*cases.scene(name, lens))
            p = cases.params()
            out[key + "_first_rgb"] = ren.render(p)
            stats[key + "_first"] = ren.stats()["device_bytes"]
            out[key + "_fill_rgb"] = ren.render(p)
            out[key + "_second_sums"] = ren.render_sums(p)
            out[key + "_second_rgb"] = ren.render(p)
            stats[key + "_second"] = ren.stats()["device_bytes"]
            p = cases.params(seed0=405)
            out[key + "_reseeded_rgb"] = ren.render(p)
            out[key + "_reseeded_fill_rgb"] = ren.render(p)
            out[key + "_reseeded_sums"] = ren.render_sums(p)
    np.savez(os.path.join(folder, "out.npz"), **out)
    with open(os.path.join(folder, "stats.json"), "w") as f:
        json.dump(stats, f)


if __name__ == "__main__":
    main()
