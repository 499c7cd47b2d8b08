"""raytrace --matte on the MI355X: the PNG's pixels equal Film.matte_coverage's grey image, on one
device and over a device list (the group film), with --progressive and --adaptive; without
--matte-samples the matte is made from the samples each pixel got; --matte and --matte-out need each
other."""
import re
import subprocess

import numpy as np
import pytest

import edge_inputs
import golden_data
import uecraytracing_amd as yk
from uecraytracing_amd.records import MATTE_SKY, make_params

pytestmark = pytest.mark.gpu

SCENE = golden_data.GOLDEN + "/final48.yks"
COMMON = ("--scene-file", SCENE, "--width", "32", "--seed0", "404")
IDS = [0, 7, MATTE_SKY, 7]


def cli(*args):
    return subprocess.run([yk.CLI_PATH, *args], capture_output=True, text=True, timeout=300)


def pixels(path, shape=(18, 32, 3)):
    rgb, W, H = golden_data.png_rgb(str(path))
    assert (H, W) == shape[:2]
    return np.frombuffer(rgb, np.uint8).reshape(shape)


def stats_line(stdout):
    m = re.search(r"^matte: pixels (\d+) uncertain (\d+) samples (\d+) of (\d+)$", stdout, re.M)
    assert m, stdout
    return tuple(int(v) for v in m.groups())


def test_cli_matte(tmp_path):
    sph, cam = edge_inputs.golden_scene("final48")
    with yk.Renderer(0) as ren:
        ren.set_scene(sph, cam)
        with ren.film(make_params(32, 18, 8, 50, 404)) as film:
            film.accumulate(8)
            image = film.resolve()
            own = film.mattes(0)[1], film.matte_coverage(IDS)
            first3 = film.mattes(3)[1], film.matte_coverage(IDS)
        with ren.film(make_params(32, 18, 16, 50, 404)) as film:  # --until 0.05 --adaptive: passes of 16, 4 at a time
            while film.accumulate_adaptive(0.05 * 0.05, 4).pixels_selected:
                pass
            lo, hi = film.count_range()
            adaptive = film.mattes(0)[1], film.matte_coverage(IDS)
    assert not np.array_equal(own[1][1], first3[1][1])
    out, matte = tmp_path / "o.png", tmp_path / "m.png"

    def written(r, want):
        assert r.returncode == 0, r.stderr
        mst, (_, grey, cst) = want
        assert np.array_equal(pixels(matte), np.repeat(grey[:, :, None], 3, axis=2))
        assert stats_line(r.stdout) == (cst["pixels_selected"], cst["pixels_uncertain"], cst["samples_selected"], mst["samples"])

    devices = ("--devices", "0,0")
    # the default N: the render's own counts
    written(cli(*COMMON, "--spp", "8", "--matte", "0,7,sky,7", "--matte-out", str(matte), str(out)), own)
    assert np.array_equal(pixels(out), image)
    written(cli(*COMMON, "--spp", "8", *devices, "--progressive", "3", "--matte=sky,7,0", "--matte-out", str(matte), str(out)), own)
    assert np.array_equal(pixels(out), image)
    written(cli(*COMMON, "--spp", "8", *devices, "--matte", "0,7,sky,7", "--matte-out", str(matte), "--matte-samples", "3",
                str(out)), first3)
    assert 4 <= lo <= hi <= 16
    written(cli(*COMMON, "--spp", "16", "--until", "0.05", "--adaptive", "--progressive", "4", "--matte", "0,7,sky",
                "--matte-out", str(matte), str(out)), adaptive)


def test_cli_matte_usage_errors(tmp_path):
    out, matte = str(tmp_path / "o.png"), str(tmp_path / "m.png")
    for bad in (("--matte", "0"), ("--matte-out", matte), ("--matte-samples", "2"),
                ("--matte", "0,x", "--matte-out", matte), ("--matte", "", "--matte-out", matte),
                ("--matte", "0", "--matte-out", matte, "--matte-samples", "9"),
                ("--matte", "0", "--matte-out", matte, "--pick", "1,1")):
        r = cli(*COMMON, "--spp", "8", *bad, out)
        assert r.returncode != 0, bad
    # an id that is no sphere of the scene: the library's refusal, after the render
    r = cli(*COMMON, "--spp", "2", "--matte", "48", "--matte-out", matte, out)
    assert r.returncode != 0 and "YK_MATTE_SKY" in r.stderr
