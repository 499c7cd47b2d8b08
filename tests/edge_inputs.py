"""Edge inputs shared by tests/test_edge_inputs.py (conditions on the CPU oracle alone) and
tests/test_gpu_edge_inputs.py (the kernels against the oracle): deep paths, scenes and cameras
scaled by powers of two across every range guard of the kernels, rays with an exactly zero
direction component, engine words that round to 1.0f, and degenerate image shapes.  Helpers and
case tables only: no tests here."""
import os

import numpy as np

import golden_data
import oracle_lib
import refscenes
from uecraytracing_amd.records import (PRECISION_FP32, PRECISION_FP64, RNG_MT19937, RNG_XOR128,
                                       Camera, D3, Sphere, make_params)

FP64, FP32 = PRECISION_FP64, PRECISION_FP32
MT, X128 = RNG_MT19937, RNG_XOR128
PREC_NAME = {FP64: "fp64", FP32: "fp32"}
RNG_NAME = {MT: "mt", X128: "x128"}


# ---- helpers ---------------------------------------------------------------------------------
def _mul3(v, f):
    return D3(*(c * f for c in v))


def scaled(spheres, cam, k):
    """The scene and its camera times 2^k: exact, so the image is the unit-scale one wherever
    neither the reference nor the kernel leaves its number format's range."""
    f = 2.0 ** k
    sph = [Sphere(_mul3(s.center, f), s.radius * f, D3(*s.albedo), s.fuzz, s.ior, s.material, 0)
           for s in spheres]
    c = Camera(_mul3(cam.origin, f), _mul3(cam.lower_left_corner, f), _mul3(cam.horizontal, f),
               _mul3(cam.vertical, f), D3(*cam.lens_u), D3(*cam.lens_v), cam.lens_radius * f)
    return sph, c


def t_min_for(k):
    """Secondary rays have unit-length directions, so their roots scale with the scene: t_min
    shrinks with it (k < 0) so that multi-bounce paths survive."""
    return 0.001 * min(1.0, 2.0 ** k)


def direction_scaled(cam, k):
    """A camera at the origin whose ray directions are 2^k times as long; geometry stays."""
    assert tuple(cam.origin) == (0.0, 0.0, 0.0)
    f = 2.0 ** k
    return Camera(D3(0.0, 0.0, 0.0), _mul3(cam.lower_left_corner, f), _mul3(cam.horizontal, f),
                  _mul3(cam.vertical, f), D3(*cam.lens_u), D3(*cam.lens_v), cam.lens_radius)


PLANAR_AXES = ("x", "y", "x-negzero-llc", "x-negzero")


def planar_camera(axis):
    """Cameras whose primary rays all lie in one coordinate plane through the origin.
    "x": d.x == +0.0 exactly (horizontal is 0, so columns repeat); "y": d.y == +0.0 (rows repeat);
    "x-negzero-llc": as "x" with lower_left_corner.x = -0.0 (the sum with +0.0 is still +0.0);
    "x-negzero": every x component -0.0, so d.x == -0.0 exactly."""
    z = D3(0.0, 0.0, 0.0)
    if axis == "x":
        return Camera(z, D3(0.0, -1.0, -1.0), D3(0.0, 0.0, 0.0), D3(0.0, 2.0, 0.0), z, z, 0.0)
    if axis == "y":
        return Camera(z, D3(-1.0, 0.0, -1.0), D3(2.0, 0.0, 0.0), D3(0.0, 0.0, 0.0), z, z, 0.0)
    if axis == "x-negzero-llc":
        return Camera(z, D3(-0.0, -1.0, -1.0), D3(0.0, 0.0, 0.0), D3(0.0, 2.0, 0.0), z, z, 0.0)
    if axis == "x-negzero":
        return Camera(z, D3(-0.0, -1.0, -1.0), D3(-0.0, 0.0, 0.0), D3(-0.0, 2.0, 0.0), z, z, 0.0)
    raise ValueError(axis)


def expected_twists(n):
    """rng_twists (yk_device.hpp): the scratch engine's 624-word twists a sample of n words needs."""
    return 1 + (n - 1) // 624 if n > 227 else 0


def origin_bound(spheres, cam):
    """ykbvh::build's origin_bound: 4 * max(|camera origin|_inf, max |c_k| + |r|)."""
    ext = max(abs(c) for c in cam.origin)
    for s in spheres:
        ext = max(ext, max(abs(c) for c in s.center) + abs(s.radius))
    return 4.0 * ext


def f32_tree_in_range(spheres, cam):
    """ykgpu_set_scene's FP32 guard: the float tree serves the scene."""
    return min(abs(s.radius) for s in spheres) >= 2.0 ** -20 and origin_bound(spheres, cam) <= 2.0 ** 20


def f64_tree_in_range(spheres, cam):
    """ykgpu_set_scene's FP64 guard: origin bound within [2^-60 max(1, D), 2^27], D
    the bound of the primary rays' direction components."""
    d = 1.0
    for k in range(3):
        d = max(d, abs(cam.lower_left_corner[k]) + abs(cam.horizontal[k]) + abs(cam.vertical[k]) +
                abs(cam.origin[k]) + abs(cam.lens_radius) * (abs(cam.lens_u[k]) + abs(cam.lens_v[k])))
    return 2.0 ** -60 * d <= origin_bound(spheres, cam) <= 2.0 ** 27


def golden_scene(name):
    return golden_data.read_scene_file(os.path.join(golden_data.GOLDEN, name + ".yks"))


def draw_counts(spheres, cam, p):
    """uint64[H, W, spp]: the engine words every sample of the (whole-image) render draws."""
    out = np.zeros((p.image_height, p.image_width, p.samples_per_pixel), np.uint64)
    arr = oracle_lib.sphere_array(spheres) if not hasattr(spheres, "_length_") else spheres
    for y in range(p.image_height):
        for x in range(p.image_width):
            for s in range(p.samples_per_pixel):
                out[y, x, s] = oracle_lib.sample(arr, cam, p, y, x, s)[1]
    return out


_oracle_cache = {}


def oracle(key, spheres, cam, p):
    """(rgb, sums, segments) of the oracle, computed once per case id and shared (read-only)."""
    if key not in _oracle_cache:
        rgb, sums, segs, _ = oracle_lib.render(spheres, cam, p, want_sums=True)
        rgb.setflags(write=False)
        sums.setflags(write=False)
        _oracle_cache[key] = (rgb, sums, segs)
    return _oracle_cache[key]


# ---- 1. deep paths ---------------------------------------------------------------------------
DEEP_W, DEEP_H, DEEP_SPP, DEEP_DEPTH, DEEP_SEED0 = 16, 9, 4, 450, 404
DEEP_CASES = [(FP64, MT), (FP32, MT), (FP64, X128)]
DEEP_IDS = [f"{PREC_NAME[p]}-{RNG_NAME[r]}" for p, r in DEEP_CASES]
# measured on the oracle (asserted by tests/test_edge_inputs.py): peak words per sample, samples
# past 1248 words (a third twist), past 1872 (a fourth), past 624 (FP32's second)
DEEP_MEASURED = {(FP64, MT): {"peak": 1960, "gt1248": 7, "gt1872": 1},
                 (FP32, MT): {"peak": 1352, "gt1248": 7, "gt624": 28}}


def deep_params(prec, rng, flags=0):
    return make_params(DEEP_W, DEEP_H, DEEP_SPP, DEEP_DEPTH, DEEP_SEED0, precision=prec, rng=rng,
                       flags=flags)


# ---- 2. scaled scenes ------------------------------------------------------------------------
SCALE_W, SCALE_H, SCALE_SPP, SCALE_DEPTH, SCALE_SEED0 = 32, 18, 4, 50, 404
_K64 = [s * k for k in (30, 99, 101, 110, 126, 135, 150, 199, 201, 240) for s in (-1, 1)]
# ... and both sides of the host guard of the FP64 tree (f64_tree_in_range): the origin bounds are
# 802 (rtiow5) and 8000 (final48)
_K64 = [-76, -72, -60, -12, 12, 14, 18] + _K64
_K32 = [-30, -24, -21, -19, -17, -16, -9, 9, 10, 11, 19, 21, 24]
SCALE_CASES = ([(FP64, "rtiow5", k) for k in _K64] + [(FP64, "final48", k) for k in _K64] +
               [(FP32, "rtiow5", k) for k in _K32] + [(FP32, "final48", k) for k in _K32 if k <= 21])
SCALE_IDS = [f"{PREC_NAME[p]}-{n}-k{k}" for p, n, k in SCALE_CASES]
SCALE_MIN_SEGMENTS_PER_SAMPLE = 2.0


def scale_case(prec, name, k, flags=0):
    """(spheres, camera, params) of one scaled-scene case."""
    sph, cam = scaled(*golden_scene(name), k)
    p = make_params(SCALE_W, SCALE_H, SCALE_SPP, SCALE_DEPTH, SCALE_SEED0, precision=prec,
                    t_min=t_min_for(k), flags=flags)
    return sph, cam, p


# ---- 3. direction scale ----------------------------------------------------------------------
DIR_W, DIR_H, DIR_SPP, DIR_DEPTH, DIR_SEED0 = 32, 18, 4, 50, 404
_D64 = [s * k for k in (30, 99, 101, 130, 160, 199, 201) for s in (-1, 1)] + [-250]
_D32 = [s * k for k in (10, 19, 21, 29) for s in (-1, 1)] + [-30]
DIR_CASES = [(FP64, k) for k in _D64] + [(FP32, k) for k in _D32]
DIR_IDS = [f"{PREC_NAME[p]}-k{k}" for p, k in DIR_CASES]


def dir_case(prec, k, flags=0):
    cam = direction_scaled(refscenes.reference_camera(), k)
    p = make_params(DIR_W, DIR_H, DIR_SPP, DIR_DEPTH, DIR_SEED0, precision=prec, flags=flags)
    return refscenes.mixed12(), cam, p


# ---- 4. planar cameras -----------------------------------------------------------------------
PLANAR_W, PLANAR_H, PLANAR_SPP, PLANAR_DEPTH, PLANAR_SEED0 = 8, 16, 4, 50, 404
PLANAR_CASES = [(prec, name, axis) for prec in (FP64, FP32) for name in ("mixed12", "rtiow5")
                for axis in PLANAR_AXES]
PLANAR_IDS = [f"{PREC_NAME[p]}-{n}-{a}" for p, n, a in PLANAR_CASES]


def planar_case(prec, name, axis, flags=0):
    sph = refscenes.mixed12() if name == "mixed12" else golden_scene(name)[0]
    p = make_params(PLANAR_W, PLANAR_H, PLANAR_SPP, PLANAR_DEPTH, PLANAR_SEED0, precision=prec,
                    flags=flags)
    return sph, planar_camera(axis), p


# ---- 5. FP32 canonical clamp -----------------------------------------------------------------
CLAMP_W, CLAMP_H, CLAMP_SPP, CLAMP_DEPTH = 4, 3, 1, 50
CLAMP_WORD = 0xFFFFFF80  # words from here up round to 2^32 in float: canonical() clamps
_X128_XYZ = (123456789, 362436069, 521288629)


def _unshift19(v):
    return v ^ (v >> 19)  # inverse of w ^ (w >> 19): 2 * 19 > 32


def xor128_seed_for_word(n, word=0xFFFFFFFF):
    """The seed whose yk::xor128 engine returns `word` as output n (0 or 1), in closed form."""
    def tt(x):
        t = (x ^ (x << 11)) & 0xFFFFFFFF
        return t ^ (t >> 8)
    w = _unshift19(word ^ tt(_X128_XYZ[n]))  # the w that output n is made from
    if n == 1:
        w = _unshift19(w ^ tt(_X128_XYZ[0]))  # ... which is output 0: back to the seeded w
    return w ^ 88675123


# mt19937 seeds found offline (a vectorised walk of the 397 seeding steps over all seeds from 0,
# the first hit of each kind)
MT_SEED_FIRST_WORD = 14784396
MT_SEED_SECOND_WORD = 2180022
# (rng, which word, engine seed of the pixel's sample, pixel y): pixel x is 0, sample 0
CLAMP_CASES = [(X128, 0, xor128_seed_for_word(0), 0), (MT, 0, MT_SEED_FIRST_WORD, 0),
               (X128, 1, xor128_seed_for_word(1), CLAMP_H - 1), (MT, 1, MT_SEED_SECOND_WORD, CLAMP_H - 1)]
CLAMP_IDS = [f"{RNG_NAME[r]}-word{n}" for r, n, _, _ in CLAMP_CASES]


def clamp_params(rng, seed, y, flags=0):
    """seed0 such that sample 0 of pixel (x = 0, y) is seeded with `seed`."""
    seed0 = (seed - y * CLAMP_W * CLAMP_SPP) & 0xFFFFFFFF
    return make_params(CLAMP_W, CLAMP_H, CLAMP_SPP, CLAMP_DEPTH, seed0, precision=FP32, rng=rng,
                       flags=flags)


# ---- 6. image shapes -------------------------------------------------------------------------
# (W, H, spp, depth, rows, cols)
SHAPES = [(1, 1, 1, 50, None, None), (1, 5, 2, 50, None, None), (5, 1, 2, 50, None, None),
          (7, 3, 1, 0, None, None), (7, 3, 3, 1, None, None),
          (4099, 3, 2, 50, None, (4090, 9, 1)),
          (65537, 3, 2, 50, (1, 1, 1), (65500, 37, 1)),
          (1000003, 2, 2, 50, None, (999990, 13, 1)),
          (17, 65537, 2, 50, (65530, 7, 1), None)]
SHAPE_CASES = [(prec,) + s for prec in (FP64, FP32) for s in SHAPES]
SHAPE_IDS = [f"{PREC_NAME[c[0]]}-{c[1]}x{c[2]}x{c[3]}-d{c[4]}" for c in SHAPE_CASES]
SHAPE_SEED0 = 404


def shape_params(prec, W, H, spp, depth, rows, cols, flags=0):
    return make_params(W, H, spp, depth, SHAPE_SEED0, precision=prec, rows=rows, cols=cols, flags=flags)
