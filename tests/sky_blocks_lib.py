"""Shared by tests/test_sky_blocks.py and tests/test_gpu_sky_blocks.py (TEST INFRASTRUCTURE ONLY): the
scenes and cameras of the sky-block tests, the classifier's driver (tests/sky_blocks_driver.cpp) and
the exact ray family of a processing block, restated in numpy from camera_ray
(uecraytracing_amd/csrc/yk_render_device.hpp)."""
import json
import math
import os
import subprocess

import numpy as np

import refscenes
from uecraytracing_amd import tiles
from uecraytracing_amd.records import Camera, D3, lambertian, metal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uecraytracing_amd", "csrc")
TOP = 1.0 - 2.0 ** -53  # the largest canonical


def look_at(origin, at, vup, vfov_deg, aspect, aperture, focus) -> Camera:
    """The book's positionable thin-lens camera as a yk_camera."""
    o, at, vup = (np.array(v, np.float64) for v in (origin, at, vup))
    h = math.tan(math.radians(vfov_deg) / 2)
    w = (o - at) / np.linalg.norm(o - at)
    u = np.cross(vup, w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    hor, ver = focus * (aspect * 2 * h) * u, focus * (2 * h) * v
    llc = o - hor / 2 - ver / 2 - focus * w
    return Camera(D3(*o), D3(*llc), D3(*hor), D3(*ver), D3(*u), D3(*v), aperture / 2)


def with_lens(cam: Camera, lens_radius: float) -> Camera:
    """cam with another lens radius; a camera without a lens basis gets its image plane's."""
    c = Camera.from_buffer_copy(cam)
    c.lens_radius = lens_radius
    if lens_radius > 0 and not any(c.lens_u) and not any(c.lens_v):
        u, v = np.array(c.horizontal), np.array(c.vertical)
        c.lens_u, c.lens_v = D3(*(u / np.linalg.norm(u))), D3(*(v / np.linalg.norm(v)))
    return c


def all_sky_scene():
    """The reference camera (at the origin, looking down -z) and one sphere behind it."""
    return [lambertian((0.0, 0.0, 5.0), 1.0, (0.5, 0.5, 0.5))], refscenes.reference_camera()


def no_sky_scene():
    """The reference scene inside a shell around the camera: every camera ray hits something."""
    return refscenes.ref4() + [metal((0.0, 0.0, 0.0), 10.0, (0.7, 0.8, 0.9))], refscenes.reference_camera()


def geometry(W, H, rows=None, cols=None):
    """The driver's tile arguments and the order stride (yk_pipeline.hip order_stride) of a tile."""
    rb, rc, rs, band = (tuple(rows) + (0,))[:4] if rows is not None else (0, H, 1, 0)
    cb, cc, cs, cband = (tuple(cols) + (0,))[:4] if cols is not None else (0, W, 1, 0)
    stride = rs if rc > 1 and band < 3 else 1
    return dict(W=W, H=H, rows=(rb, rc, rs, band), cols=(cb, cc, cs, cband), stride=stride)


def tile_geometries(W, H):
    """The whole image, a row tile and a column tile of a 2-way split (uecraytracing_amd/tiles.py)."""
    return {"whole": geometry(W, H), "rows1of2": geometry(W, H, rows=tiles.tile_rows(1, 2, H)),
            "cols0of2": geometry(W, H, cols=tiles.tile_cols(0, 2, W))}


def banded(begin, stride, band, t):
    return begin + (((t >> band) * stride) << band) + (t & ((1 << band) - 1))


def build_driver(workdir, sanitize=False):
    exe = os.path.join(str(workdir), "sky_driver_san" if sanitize else "sky_driver")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", *flags, "-o", exe,
                    os.path.join(ROOT, "tests", "sky_blocks_driver.cpp"), os.path.join(CSRC, "yk_bvh.cpp")], check=True)
    return exe


def write_scene(path, spheres, cam: Camera):
    with open(path, "w") as f:
        vals = [*cam.origin, *cam.lower_left_corner, *cam.horizontal, *cam.vertical, *cam.lens_u, *cam.lens_v,
                cam.lens_radius]
        f.write("camera " + " ".join(repr(float(v)) for v in vals) + "\n")
        for s in spheres:
            f.write(" ".join(repr(float(v)) for v in (*s.center, s.radius)) + "\n")


def classify(exe, scene_path, g):
    """The driver's block grid for geometry g: dict with tw, th, bx, by, flags (row-major by block row)."""
    args = [exe, scene_path, g["W"], g["H"], *g["rows"], *g["cols"], g["stride"]]
    out = subprocess.run([str(a) for a in args], check=True, capture_output=True, text=True).stdout
    return json.loads(out)


def block_pixels(g, grid, i, j):
    """(xs, ys): image coordinates of the pixels of block column i, block row j."""
    tw, th = grid["tw"], grid["th"]
    (rb, rc, rs, band), (cb, cc, cs, cband) = g["rows"], g["cols"]
    xs = [banded(cb, cs, cband, t) for t in range(i * tw, min(cc, (i + 1) * tw))]
    ys = [banded(rb, rs, band, t) for t in range(j * th, min(rc, (j + 1) * th))]
    return xs, ys


def family_rays(cam: Camera, W, H, xs, ys, n, rng):
    """n rays of the family of the pixels xs x ys: random pixels, jitters and lens points, then the
    extremes — the corner pixels at uc, vc in {0, 1 - 2^-53}, each with lens points on the rim.
    Every statement is camera_ray's, one IEEE operation per element."""
    xs, ys = np.array(xs, np.float64), np.array(ys, np.float64)
    x, y = rng.choice(xs, n), rng.choice(ys, n)
    uc, vc = rng.random(n), rng.random(n)
    r, phi = np.sqrt(rng.random(n)), rng.random(n) * 2 * np.pi
    px, py = r * np.cos(phi), r * np.sin(phi)
    ex = [(cx, cy, a, b) for cx in (xs[0], xs[-1]) for cy in (ys[0], ys[-1]) for a in (0.0, TOP) for b in (0.0, TOP)]
    rim = [(math.cos(t) * (1 - 1e-12), math.sin(t) * (1 - 1e-12)) for t in np.arange(8) * (math.pi / 4)]
    k = len(ex) * len(rim)  # 128 rays at the extremes
    x[:k], y[:k] = np.repeat([e[0] for e in ex], len(rim)), np.repeat([e[1] for e in ex], len(rim))
    uc[:k], vc[:k] = np.repeat([e[2] for e in ex], len(rim)), np.repeat([e[3] for e in ex], len(rim))
    px[:k], py[:k] = np.tile([p[0] for p in rim], len(ex)), np.tile([p[1] for p in rim], len(ex))
    assert (px * px + py * py < 1.0).all()
    u = (x + uc) / np.float64(W)
    v = (((np.float64(H) - y) - 1.0) + vc) / np.float64(H)
    o = [np.full(n, np.float64(c)) for c in cam.origin]
    d = [((np.float64(cam.lower_left_corner[k]) + np.float64(cam.horizontal[k]) * u) +
          np.float64(cam.vertical[k]) * v) - o[k] for k in range(3)]
    if cam.lens_radius > 0:
        rx, ry = px * np.float64(cam.lens_radius), py * np.float64(cam.lens_radius)
        off = [np.float64(cam.lens_u[k]) * rx + np.float64(cam.lens_v[k]) * ry for k in range(3)]
        o = [o[k] + off[k] for k in range(3)]
        d = [d[k] - off[k] for k in range(3)]
    return np.stack(o, -1), np.stack(d, -1)
