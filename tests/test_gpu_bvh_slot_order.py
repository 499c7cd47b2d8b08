"""The camera-ordered wide nodes change no pixel — on the MI355X.

ykgpu_set_scene orders the slots of every wide node front to back from the camera's origin
(yk_bvh.hpp SlotOrder), so every camera position builds another tree.  The BVH only
culls: with the camera at its usual place, inside the sphere cloud and far outside it, the float64
per-pixel sums equal those of the exact linear scan of the same call bit for bit, in FP64 and FP32.
The shallow checked stack (the stack5 test build) overflows on an ordered tree as on any other and
still equals the product library.
"""
import json
import os
import subprocess
import sys

import pytest

import golden_data
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd.records import FLAG_LINEAR_SCAN, PRECISION_FP32, PRECISION_FP64, Camera, D3, make_params

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def moved(cam: Camera, t) -> Camera:
    """The camera translated by t: the same rays from another origin."""
    o = tuple(a + b for a, b in zip(cam.origin, t))
    llc = tuple(a + b for a, b in zip(cam.lower_left_corner, t))
    return Camera(D3(*o), D3(*llc), cam.horizontal, cam.vertical, cam.lens_u, cam.lens_v, cam.lens_radius)


def cameras(name, cam):
    o = tuple(cam.origin)
    if name == "dupes":
        # the reference camera at the origin looks down -z at the six spheres at (0, 0, -1), radius
        # 0.5; "inside": a corner of their boxes, outside the spheres (inside them the image is black)
        return {"usual": cam, "inside": moved(cam, (0.45, 0.45, -0.55)), "far": moved(cam, (0.0, 40.0, 300.0))}
    # final48 / glass48: the camera at (13, 2, 3) looks at the cloud around the origin
    return {"usual": cam, "inside": moved(cam, tuple(-0.9 * v for v in o)), "far": moved(cam, tuple(20.0 * v for v in o))}


# scene -> (spheres, camera, W, H, spp, depth)
def case(name):
    if name == "dupes":
        return refscenes.dupes(), refscenes.reference_camera(), 16, 9, 2, 50
    sph, cam = golden_data.read_scene_file(os.path.join(GOLDEN, name + ".yks"))
    return sph, cam, 32, 18, 4, 200 if name == "glass48" else 50


@pytest.fixture(scope="module")
def ren():
    r = yk.Renderer(0)
    yield r
    r.close()


@pytest.mark.parametrize("where", ("usual", "inside", "far"))
@pytest.mark.parametrize("name", ("final48", "glass48", "dupes"))
def test_ordered_tree_equals_linear_scan(ren, name, where):
    sph, cam, W, H, spp, depth = case(name)
    ren.set_scene(sph, cameras(name, cam)[where])
    for prec in (PRECISION_FP64, PRECISION_FP32):
        tree = ren.render_sums(make_params(W, H, spp, depth, 404, precision=prec))
        scan = ren.render_sums(make_params(W, H, spp, depth, 404, precision=prec, flags=FLAG_LINEAR_SCAN))
        assert tree.tobytes() == scan.tobytes(), (name, where, prec)
        assert float(abs(tree).sum()) > 0.0


_CODE = r'''
import hashlib, json, os, sys
sys.path.insert(0, os.environ["YK_ROOT"])
sys.path.insert(0, os.path.join(os.environ["YK_ROOT"], "tests"))
import golden_data
import uecraytracing_amd as yk
from uecraytracing_amd.records import make_params
sph, cam = golden_data.read_scene_file(os.path.join(os.environ["YK_ROOT"], "tests", "golden", "final48.yks"))
with yk.Renderer(0) as r:
    r.set_scene(sph, cam)
    sums = r.render_sums(make_params(32, 18, 4, 50, 404, flags=1))  # counting instance
    st = r.stats()
print(json.dumps({"sha": hashlib.sha256(sums.tobytes()).hexdigest(), "linear_scans": st["linear_scans"]}))
'''


def test_shallow_stack_build_on_the_ordered_tree():
    root = yk.LIB_DIR
    repo = os.path.dirname(os.path.dirname(root))
    res = {}
    for name, lib in (("product", os.path.join(root, "libykgpu.so")),
                      ("stack5", os.path.join(root, "abl", "libykgpu_stack5.so"))):
        assert os.path.exists(lib), f"{lib}: built by uecraytracing_amd/csrc/Makefile (all)"
        env = dict(os.environ, YKGPU_LIB_OVERRIDE=lib, YK_ROOT=repo)
        pr = subprocess.run([sys.executable, "-c", _CODE], env=env, capture_output=True, text=True, timeout=120)
        assert pr.returncode == 0, pr.stderr[-2000:]
        res[name] = json.loads([ln for ln in pr.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["stack5"]["sha"] == res["product"]["sha"]
    assert res["product"]["linear_scans"] == 0 < res["stack5"]["linear_scans"]  # the checked path really ran
