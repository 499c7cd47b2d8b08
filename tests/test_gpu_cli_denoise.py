"""raytrace --denoise on the MI355X: the PNG holds Film.denoise's RGB8, for the final image and for
a --progressive run stopped early, with and without the parameter options; without --denoise the
program writes the bytes it always wrote (the reference's constexpr image)."""
import subprocess

import numpy as np
import pytest

import golden_data
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd.records import make_params

pytestmark = pytest.mark.gpu


def cli(*args):
    return subprocess.run([yk.CLI_PATH, *args], capture_output=True, text=True, timeout=300)


def pixels(path, shape=(9, 16, 3)):
    rgb, W, H = golden_data.png_rgb(str(path))
    assert (H, W) == shape[:2]
    return np.frombuffer(rgb, np.uint8).reshape(shape)


def test_cli_denoise_writes_the_films_filtered_image(tmp_path):
    common = ("--scene", "ref4", "--width", "16", "--spp", "8", "--seed0", "404")
    out = tmp_path / "o.png"
    with yk.Renderer(0) as ren:
        ren.set_scene(refscenes.ref4(), refscenes.reference_camera())
        with ren.film(make_params(16, 9, 8, 50, 404)) as film:
            film.accumulate(4)
            early = film.denoise(want_mean=False)[1]
            film.accumulate(4)
            final = film.denoise(want_mean=False)[1]
            tuned = film.denoise(radius=2, patch=0, k2=0.25, want_mean=False)[1]
            raw = film.resolve()
    assert not np.array_equal(final, raw) and not np.array_equal(final, tuned)
    # without film options: a one-chunk film
    r = cli(*common, "--denoise", str(out))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(pixels(out), final)
    r = cli(*common, "--denoise", "--denoise-radius", "2", "--denoise-patch", "0", "--denoise-k2", "0.25", str(out))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(pixels(out), tuned)
    # a progressive run stopped after its first chunk leaves that chunk's filtered image
    r = cli(*common, "--denoise", "--progressive", "4", "--stop-after", "1", str(out))
    assert r.returncode == 0 and "stopped at 4 of 8 samples" in r.stdout.splitlines(), r.stdout + r.stderr
    assert np.array_equal(pixels(out), early)
    r = cli(*common, "--denoise", "--progressive", "4", str(out))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(pixels(out), final)
    # the same run without --denoise is the raw image, as before
    r = cli(*common, str(out))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(pixels(out), raw)
    # one sample per pixel cannot be filtered: the library's error is the run's
    r = cli("--width", "16", "--spp", "1", "--seed0", "404", "--denoise", str(tmp_path / "no.png"))
    assert r.returncode == 1 and "two samples" in r.stderr and not (tmp_path / "no.png").exists()


def test_cli_without_denoise_writes_the_constexpr_image(tmp_path):
    out = tmp_path / "c.png"
    r = cli("--width", "16", "--spp", "2", "--seed0", "404", str(out))
    assert r.returncode == 0, r.stderr
    assert golden_data.sha(pixels(out)) == golden_data.manifest()["constexpr_build"]["rgb_sha256"]
