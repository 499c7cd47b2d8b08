"""raytrace --aov and --denoise-features on the MI355X: the three feature PNGs and the guided image,
decoded, equal the numpy yardstick's bytes (film_features_ref) at 16x9; --denoise-* still set the
colour side and --feature-grid the grid of both."""
import subprocess

import numpy as np
import pytest

import film_denoise_ref as fdr
import film_features_ref as ffr
import film_ref
import golden_data
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd.records import make_params

pytestmark = pytest.mark.gpu

CAM = refscenes.reference_camera()


def cli(*args):
    return subprocess.run([yk.CLI_PATH, *args], capture_output=True, text=True, timeout=300)


def pixels(path, shape=(9, 16, 3)):
    rgb, W, H = golden_data.png_rgb(str(path))
    assert (H, W) == shape[:2]
    return np.frombuffer(rgb, np.uint8).reshape(shape)


def test_cli_writes_the_feature_images_and_the_guided_image(tmp_path):
    common = ("--scene", "ref4", "--width", "16", "--spp", "8", "--seed0", "404")
    p = make_params(16, 9, 8, 50, 404)
    scene = refscenes.ref4()
    S, Q = film_ref.prefixes(film_ref.colours(scene, CAM, p))
    out, prefix = tmp_path / "o.png", tmp_path / "f"

    def aov(grid):
        albedo, normal, depth = ffr.aov_images(ffr.features(scene, CAM, p, grid)[0])
        assert np.array_equal(pixels(str(prefix) + ".albedo.png"), albedo)
        assert np.array_equal(pixels(str(prefix) + ".normal.png"), normal)
        assert np.array_equal(pixels(str(prefix) + ".depth.png"), np.repeat(depth[:, :, None], 3, axis=2))
        return albedo, normal, depth

    r = cli(*common, "--denoise-features", "--aov", str(prefix), str(out))
    assert r.returncode == 0, r.stderr
    guided = fdr.to_rgb8(ffr.denoise_guided(S[8], Q[8], 8, scene, CAM, p))
    assert np.array_equal(pixels(out), guided)
    albedo, normal, depth = aov(2)
    assert tuple(albedo[0, 0]) == (255, 255, 255) and tuple(normal[0, 0]) == (128, 128, 128) and depth[0, 0] == 0  # the sky
    assert len(np.unique(albedo.reshape(-1, 3), axis=0)) > 4 and depth.max() > 100
    # the colour side's options and the grid still apply
    r = cli(*common, "--denoise-features", "--denoise-radius", "2", "--denoise-patch", "0", "--denoise-k2", "0.25",
            "--feature-grid", "1", "--aov", str(prefix), str(out))
    assert r.returncode == 0, r.stderr
    tuned = fdr.to_rgb8(ffr.denoise_guided(S[8], Q[8], 8, scene, CAM, p, colour=dict(radius=2, patch=0, k2=0.25),
                                           feat=dict(grid=1)))
    assert np.array_equal(pixels(out), tuned) and not np.array_equal(tuned, guided)
    aov(1)
    # --aov alone leaves the image the raw mean
    r = cli(*common, "--aov", str(prefix), str(out))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(pixels(out), film_ref.to_color3b(S[8], 8))
    aov(2)
