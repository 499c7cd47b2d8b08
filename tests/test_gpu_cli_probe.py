"""raytrace --probe on the MI355X: the samples of one pixel through the radiance query.  The folded
sum it prints (%.17g: every double round-trips) is that pixel of render_sums, the RGB8 triple that
pixel of the rendered image, the per-sample lines carry the restatement's records (radiance_ref),
and no image is rendered.  (The argument errors need no device: test_radiance_ref.py.)"""
import subprocess

import numpy as np
import pytest

import radiance_ref as rr
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd import records
from uecraytracing_amd.records import make_params

pytestmark = pytest.mark.gpu

CAM = refscenes.reference_camera()
W, H, SPP, SEED0 = 64, 36, 5, 404
HOW = {rr.SKY: "sky", rr.ABSORBED: "absorbed", rr.DEPTH: "depth", rr.OOD: "out-of-domain"}


def cli(*args):
    return subprocess.run([yk.CLI_PATH, *args], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def rendered():
    p = make_params(W, H, SPP, 50, SEED0)
    with yk.Renderer(0) as ren:
        ren.set_scene(refscenes.ref4(), CAM)
        return p, ren.render_sums(p), ren.render(p)


@pytest.mark.parametrize("x,y", [(32, 18), (10, 17), (40, 33), (0, 0)])
def test_probe_prints_the_pixel_of_the_render(tmp_path, rendered, x, y):
    p, sums, image = rendered
    r = cli("--scene", "ref4", "--width", str(W), "--spp", str(SPP), "--seed0", str(SEED0), "--probe", f"{x},{y}")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == SPP + 2 and "rendering" not in r.stdout and not list(tmp_path.iterdir())
    v = lambda a: "(" + ", ".join("%.17g" % c for c in a) + ")"
    assert lines[SPP] == "sum " + v(sums[y, x])
    assert lines[SPP + 1] == "rgb %d %d %d" % tuple(image[y, x])
    want = rr.radiance(refscenes.ref4(), rr.camera_rays(CAM, p, [y] * SPP, [x] * SPP, range(SPP)))
    for s, rec in enumerate(want):
        how = HOW[int(rec["flags"]) & ~rr.FALLBACK]
        assert lines[s] == f"sample {s}: colour {v(rec['colour'])} words {rec['words']} segments {rec['segments']} end {how}"
    acc = np.zeros(3)
    for rec in want:
        acc = acc + rec["colour"]
    assert acc.tobytes() == np.ascontiguousarray(sums[y, x]).tobytes()
    # an output file on the command line is not written
    out = tmp_path / "o.png"
    r2 = cli("--scene", "ref4", "--width", str(W), "--spp", str(SPP), "--seed0", str(SEED0), f"--probe={x},{y}", str(out))
    assert r2.returncode == 0 and r2.stdout == r.stdout and not out.exists()

