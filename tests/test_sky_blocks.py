"""The sky-block classifier (uecraytracing_amd/csrc/yk_sky.hpp), checked on the CPU.

A flagged block must be SOUND: no ray of its family — any jitter over any of its pixels, any lens
point — hits any sphere for any t >= 0.  Every flagged block of every case gets 2,000 rays of its
exact family (sky_blocks_lib.family_rays: 128 at the extremes — corner pixels, canonicals 0 and
1 - 2^-53, lens points on the rim — the rest random) through the closest-hit yardstick
(tests/cast_ref.py) with t_min = 0; none may hit.

And it must not be vacuous.  Measured on the final scene (pinhole rays through the pixel centres,
cast_ref): 16.4% of the pixels of the 72x40 image see only sky, but the silhouette of the three large
spheres and the horizon, 8.5 pixel rows down, leave only 4 of its 45 blocks (8.9%) without a hit —
3 of 40 at 64x36 — and with the scene's lens (0.005 rad, half a pixel there) none of them by a
margin.  One tenth of the blocks at 72x40 is therefore out of reach of any sound classifier; the
share is asserted where the pixel-level estimate of 13-14% was made, at 480x270 (2,040 blocks; this
classifier flags 221, 10.8%; 12.7% of the 32,400 blocks of 1920x1080), and at 72x40 on the same
spheres seen by a camera pitched up, where the blocks are small against the sky.

A small driver (tests/sky_blocks_driver.cpp) is compiled against yk_bvh.cpp alone: no GPU.
"""
import os
import subprocess

import numpy as np
import pytest

import cast_ref
import refscenes
import sky_blocks_lib as sbl
import uecraytracing_amd as yk
from uecraytracing_amd.records import lambertian

ROOT = sbl.ROOT
SCENE_FILES = {"rtiow5": os.path.join(ROOT, "uecraytracing_amd", "scenes", "rtiow5.yks"),
               "final48": os.path.join(ROOT, "tests", "golden", "final48.yks"),
               "final_seed42": os.path.join(ROOT, "uecraytracing_amd", "scenes", "final_seed42.yks")}
SIZES = ((72, 40), (64, 36))
RAYS = 2000


def pitched(lens):
    """The final scenes' viewpoint looking up over the spheres: sky above a ragged silhouette."""
    return sbl.look_at((13, 2, 3), (0, 4.5, 0), (0, 1, 0), 40.0, 16 / 9, 2 * lens, 10.0)


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    d = tmp_path_factory.mktemp("sky_blocks")
    exe = sbl.build_driver(d)
    count = [0]

    def run(spheres, cam, g, driver=exe):
        count[0] += 1
        path = str(d / f"scene{count[0]}.txt")
        sbl.write_scene(path, spheres, cam)
        return sbl.classify(driver, path, g)

    run.dir = d
    return run


def check_sound(spheres, cam, g, grid, seed=1):
    """Every flagged block of the grid: RAYS rays of its family, none may hit.  Returns the count."""
    rng = np.random.default_rng(seed)
    os_, ds, owner = [], [], []
    for b, f in enumerate(grid["flags"]):
        if not f:
            continue
        xs, ys = sbl.block_pixels(g, grid, b % grid["bx"], b // grid["bx"])
        o, d = sbl.family_rays(cam, g["W"], g["H"], xs, ys, RAYS, rng)
        os_.append(o), ds.append(d), owner.append(np.full(RAYS, b))
    if not os_:
        return 0
    rec = cast_ref.cast(list(spheres), np.concatenate(os_), np.concatenate(ds), 0.0)
    assert (rec["flags"] == 0).all(), f"rays of flagged blocks {sorted(set(np.concatenate(owner)[rec['flags'] != 0]))} hit"
    return len(os_)


def scene_cases():
    for name, path in SCENE_FILES.items():
        spheres, cam = yk.read_scene(path)
        for lens in (0.0, 0.05):
            yield f"{name}-lens{lens}", list(spheres), sbl.with_lens(cam, lens)
    final = list(yk.read_scene(SCENE_FILES["final_seed42"])[0])
    for lens in (0.0, 0.05):
        yield f"final_seed42-pitched-lens{lens}", final, pitched(lens)


@pytest.mark.parametrize("case", list(scene_cases()), ids=lambda c: c[0])
def test_flagged_blocks_are_sound(env, case):
    _, spheres, cam = case
    flagged = 0
    for W, H in SIZES:
        for gname, g in sbl.tile_geometries(W, H).items():
            grid = env(spheres, cam, g)
            assert len(grid["flags"]) == grid["bx"] * grid["by"]
            flagged += check_sound(spheres, cam, g, grid)
    if "pitched" in case[0]:
        assert flagged > 0


def test_not_vacuous_on_the_final_scene(env):
    spheres, cam = yk.read_scene(SCENE_FILES["final_seed42"])
    grid = env(list(spheres), cam, sbl.geometry(480, 270))
    assert 10 * sum(grid["flags"]) >= len(grid["flags"]), (sum(grid["flags"]), len(grid["flags"]))
    # the named scene and camera at 72x40 and 64x36: what is reachable there — without the lens the
    # three blocks of the top row clear of the spheres' silhouette (pinhole truth: 4 and 3), with the
    # scene's lens none by a margin, so no number is set for it
    for (w, h) in SIZES:
        grid = env(list(spheres), sbl.with_lens(cam, 0.0), sbl.geometry(w, h))
        assert sum(grid["flags"]) >= 3, (w, h, sum(grid["flags"]))
    # ... and at 72x40 on the same spheres under the pitched camera, with the scene's lens
    g = sbl.geometry(72, 40)
    grid = env(list(spheres), pitched(0.05), g)
    assert 10 * sum(grid["flags"]) >= len(grid["flags"]), (sum(grid["flags"]), len(grid["flags"]))
    # what the whole image flags, its tiles flag too (a tile's blocks are other rectangles: about as many)
    for gname, gt in sbl.tile_geometries(72, 40).items():
        gridt = env(list(spheres), pitched(0.05), gt)
        assert 20 * sum(gridt["flags"]) >= len(gridt["flags"]), (gname, sum(gridt["flags"]), len(gridt["flags"]))


@pytest.mark.parametrize("lens", (0.0, 0.05))
def test_all_sky_and_no_sky(env, lens):
    for W, H in SIZES:
        for g in sbl.tile_geometries(W, H).values():
            spheres, cam = sbl.all_sky_scene()
            grid = env(spheres, sbl.with_lens(cam, lens), g)
            assert all(grid["flags"]), "a sphere behind the camera: every block is sky"
            check_sound(spheres, sbl.with_lens(cam, lens), g, grid)
            spheres, cam = sbl.no_sky_scene()
            grid = env(spheres, sbl.with_lens(cam, lens), g)
            assert not any(grid["flags"]), "the camera inside a sphere: no block is sky"


def test_degenerate_cameras_flag_nothing(env):
    spheres, cam = sbl.all_sky_scene()
    g = sbl.geometry(72, 40)
    for field, value in (("horizontal", (0.0, 0.0, 0.0)), ("vertical", (0.0, 0.0, 0.0)),
                         ("lower_left_corner", (float("nan"), 0.0, 0.0)), ("origin", (float("inf"), 0.0, 0.0)),
                         ("horizontal", (1e308, 1e308, 0.0))):
        c = sbl.with_lens(cam, 0.0)
        setattr(c, field, type(c.origin)(*value))
        assert not any(env(spheres, c, g)["flags"]), field
    # a lens wider than the focus distance: no bound on where a ray can go
    assert not any(env(spheres, sbl.with_lens(cam, 2.0), g)["flags"])


@pytest.mark.parametrize("lens", (0.0, 0.05))
def test_edge_inputs(env, lens):
    """A sphere tangent to a block's pinhole pyramid (from outside, and pushed in and out by a few
    ulps and by 1e-6), and one just behind the camera plane: whatever is flagged must be sound, and
    the sphere well outside must leave its neighbour block flagged."""
    cam = sbl.with_lens(refscenes.reference_camera(), lens)
    W, H = 72, 40
    g = sbl.geometry(W, H)
    # the right side plane of block column 3: through the origin and the image column x = 32
    u = 32 / W
    edge = np.array(cam.lower_left_corner) + np.array(cam.horizontal) * u  # bottom of that column
    n = np.cross(np.array(cam.vertical), edge)  # normal of the plane through O, edge, edge + vertical
    n /= np.linalg.norm(n)
    n = n if n[0] > 0 else -n  # pointing right, away from the block
    along = edge + np.array(cam.vertical) * 0.5
    base = along / np.linalg.norm(along) * 3.0
    r = 0.25
    for k, eps in enumerate((0.0, 4e-16, -4e-16, 1e-6, -1e-6, 0.2)):
        spheres = [lambertian(tuple(base + n * (r + eps)), r, (0.5, 0.5, 0.5))]
        grid = env(spheres, cam, g)
        check_sound(spheres, cam, g, grid, seed=10 + k)
        left = [grid["flags"][j * grid["bx"] + 3] for j in range(grid["by"])]
        if eps == 0.2 and lens == 0.0:
            assert all(left), "a sphere 0.2 outside the plane hides nothing of block column 3"
        if eps <= 0:
            assert not all(left), "a sphere touching the plane from inside must unflag a block"
    # behind the camera plane z = 0 (the camera looks down -z), touching it or nearly
    for k, gap in enumerate((0.0, 1e-12, 1e-6, 1e-3, 0.5)):
        spheres = [lambertian((0.01, -0.02, 1.0 + gap), 1.0, (0.5, 0.5, 0.5))]
        grid = env(spheres, cam, g)
        check_sound(spheres, cam, g, grid, seed=20 + k)
        if gap >= (1e-3 if lens == 0.0 else 0.5):  # (the bound takes the lens as a ball around the origin)
            assert all(grid["flags"])


def test_driver_under_sanitizers(env):
    """The classifier once under AddressSanitizer and UBSan, as a stand-alone program."""
    exe = sbl.build_driver(env.dir, sanitize=True)
    spheres, cam = yk.read_scene(SCENE_FILES["final_seed42"])
    for g in (sbl.geometry(72, 40), sbl.tile_geometries(64, 36)["rows1of2"], sbl.tile_geometries(64, 36)["cols0of2"],
              sbl.geometry(257, 131)):
        a, b = env(list(spheres), cam, g, driver=exe), env(list(spheres), cam, g)
        assert a["flags"] == b["flags"]
