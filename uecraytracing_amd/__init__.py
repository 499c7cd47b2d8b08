"""uecraytracing_amd — MI355X (gfx950) renderer for the per-pixel sampling loop of
yaito3014/UECRayTracing.

The product is the C-ABI library ``uecraytracing_amd/lib/libykgpu.so`` (include/ykgpu.h) and the
drop-in CLI ``uecraytracing_amd/lib/raytrace``.  This module is a thin ctypes view of that
library for tests and the benchmark: it has NO fallback — if the library or a GPU is missing,
every render raises.
"""
from __future__ import annotations

import ctypes
import os
import weakref

import numpy as np

from . import records
from .records import CastStats, Hit, Ray, PathRay, GatherParams, GatherStats, RadianceParams, RadianceStats, Camera, DenoiseParams, DenoiseStats, FeatureParams, FilmPass, GroupDenoiseStats, GuidedStats, FilmStats, MatteCoverageStats, MattePixel, MatteStats, SampledFeaturesStats, RenderParams, RenderStats, Sphere, make_params, sphere_array

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(PKG_DIR, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libykgpu.so")
# tools/ablate.py loads timing-only variants through this override; tests never set it
LIB_PATH = os.environ.get("YKGPU_LIB_OVERRIDE", LIB_PATH)
CLI_PATH = os.path.join(LIB_DIR, "raytrace")

EXPORTS = (
    "ykgpu_abi_version", "ykgpu_last_error", "ykgpu_device_count", "ykgpu_context_create",
    "ykgpu_context_destroy", "ykgpu_set_scene", "ykgpu_render", "ykgpu_render_async",
    "ykgpu_render_sums", "ykgpu_render_trace", "ykgpu_get_stats", "ykgpu_math_sqrt", "ykgpu_math_sqrt_f32", "ykgpu_math_div", "ykgpu_math_div_f32", "yk_camera_reference", "yk_camera_look",
    "yk_scene_build", "yk_scene_write", "yk_scene_read", "yk_image_height_for",
    "ykgpu_group_create", "ykgpu_group_destroy", "ykgpu_group_size", "ykgpu_group_set_scene",
    "ykgpu_group_render", "ykgpu_group_get_stats", "ykgpu_render_devices",
    "ykgpu_film_create", "ykgpu_film_destroy", "ykgpu_film_params", "ykgpu_film_accumulate",
    "ykgpu_film_resolve", "ykgpu_film_read", "ykgpu_film_write", "ykgpu_film_error",
    "yk_film_save", "yk_film_load", "yk_scene_hash",
    "ykgpu_film_accumulate_adaptive", "ykgpu_film_counts", "ykgpu_film_write_counts",
    "yk_film_save_counts", "yk_film_load_counts",
    "yk_denoise_defaults", "ykgpu_film_denoise",
    "yk_guided_defaults", "ykgpu_film_features", "ykgpu_film_denoise_guided",
    "ykgpu_group_film_create", "ykgpu_group_film_destroy", "ykgpu_group_film_params",
    "ykgpu_group_film_accumulate", "ykgpu_group_film_accumulate_adaptive", "ykgpu_group_film_resolve",
    "ykgpu_group_film_read", "ykgpu_group_film_write", "ykgpu_group_film_counts", "ykgpu_group_film_write_counts",
    "ykgpu_group_film_error", "ykgpu_group_film_features", "ykgpu_group_film_denoise",
    "ykgpu_group_film_denoise_guided",
    "yk_guided_sampled_defaults", "ykgpu_film_features_sampled", "ykgpu_film_denoise_guided_sampled",
    "ykgpu_group_film_features_sampled", "ykgpu_group_film_denoise_guided_sampled",
    "ykgpu_film_mattes", "ykgpu_film_matte_coverage", "ykgpu_group_film_mattes", "ykgpu_group_film_matte_coverage",
    "ykgpu_cast_rays", "ykgpu_cast_rays_async", "ykgpu_cast_get_stats",
    "ykgpu_radiance_rays", "ykgpu_radiance_rays_async", "ykgpu_radiance_get_stats", "yk_camera_sample_ray",
    "yk_camera_sample_rays",
    "ykgpu_gather_points", "ykgpu_gather_points_async", "ykgpu_gather_get_stats", "yk_gather_sample_ray",
    "yk_gather_sample_rays",
)
ABI_VERSION = 11
SCENE_DIR = os.path.join(PKG_DIR, "scenes")  # committed scene files of the BASELINE configs

_lib = None


class YkError(RuntimeError):
    pass


def load_library():
    """Loads libykgpu.so (built by __graft_entry__.build / `make -C uecraytracing_amd/csrc`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise YkError(f"{LIB_PATH} is missing: build it with `make -C uecraytracing_amd/csrc` "
                      "(there is no CPU fallback)")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64/libhsa-runtime64
    # (soname libamdhip64.so.7, like /opt/rocm's).  If torch is importable it is loaded FIRST
    # so that libykgpu.so binds to the already-loaded runtime instead of pulling in a second
    # copy, which would leave whichever initialises second without a GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    P, c = ctypes.POINTER, ctypes
    sig = {
        "ykgpu_abi_version": ([], c.c_uint32),
        "ykgpu_last_error": ([], c.c_char_p),
        "ykgpu_device_count": ([P(c.c_int)], c.c_int),
        "ykgpu_context_create": ([c.c_int, P(c.c_void_p)], c.c_int),
        "ykgpu_context_destroy": ([c.c_void_p], c.c_int),
        "ykgpu_set_scene": ([c.c_void_p, P(Sphere), c.c_uint32, P(Camera)], c.c_int),
        "ykgpu_render": ([c.c_void_p, P(RenderParams), c.c_void_p], c.c_int),
        "ykgpu_render_async": ([c.c_void_p, P(RenderParams), c.c_void_p, c.c_void_p], c.c_int),
        "ykgpu_render_sums": ([c.c_void_p, P(RenderParams), c.c_void_p], c.c_int),
        "ykgpu_render_trace": ([c.c_void_p, P(RenderParams), c.c_uint32, c.c_void_p, c.c_void_p], c.c_int),
        "ykgpu_get_stats": ([c.c_void_p, P(RenderStats)], c.c_int),
        "ykgpu_math_sqrt": ([c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint64], c.c_int),
        "ykgpu_math_sqrt_f32": ([c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint64], c.c_int),
        "ykgpu_math_div": ([c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint64], c.c_int),
        "ykgpu_math_div_f32": ([c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint64], c.c_int),
        "yk_camera_reference": ([P(Camera)], c.c_int),
        "yk_camera_look": ([P(Camera), P(c.c_double), P(c.c_double), P(c.c_double), c.c_double,
                            c.c_double, c.c_double, c.c_double], c.c_int),
        "yk_scene_build": ([c.c_char_p, c.c_uint32, P(Sphere), c.c_uint32, P(c.c_uint32),
                            P(Camera)], c.c_int),
        "yk_scene_write": ([c.c_char_p, P(Sphere), c.c_uint32, P(Camera)], c.c_int),
        "yk_scene_read": ([c.c_char_p, P(Sphere), c.c_uint32, P(c.c_uint32), P(Camera)], c.c_int),
        "yk_image_height_for": ([c.c_uint32], c.c_uint32),
        "ykgpu_group_create": ([P(c.c_int), c.c_uint32, P(c.c_void_p)], c.c_int),
        "ykgpu_group_destroy": ([c.c_void_p], c.c_int),
        "ykgpu_group_size": ([c.c_void_p, P(c.c_uint32)], c.c_int),
        "ykgpu_group_set_scene": ([c.c_void_p, P(Sphere), c.c_uint32, P(Camera)], c.c_int),
        "ykgpu_group_render": ([c.c_void_p, P(RenderParams), c.c_void_p], c.c_int),
        "ykgpu_group_get_stats": ([c.c_void_p, c.c_int, P(RenderStats)], c.c_int),
        "ykgpu_render_devices": ([P(c.c_int), c.c_uint32, P(Sphere), c.c_uint32, P(Camera),
                                  P(RenderParams), c.c_void_p], c.c_int),
        "ykgpu_film_create": ([c.c_void_p, P(RenderParams), P(c.c_void_p)], c.c_int),
        "ykgpu_film_destroy": ([c.c_void_p], c.c_int),
        "ykgpu_film_params": ([c.c_void_p, P(RenderParams)], c.c_int),
        "ykgpu_film_accumulate": ([c.c_void_p, c.c_uint32], c.c_int),
        "ykgpu_film_resolve": ([c.c_void_p, c.c_void_p], c.c_int),
        "ykgpu_film_read": ([c.c_void_p, c.c_void_p, c.c_void_p, P(c.c_uint32)], c.c_int),
        "ykgpu_film_write": ([c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint32], c.c_int),
        "ykgpu_film_error": ([c.c_void_p, c.c_double, c.c_void_p, P(FilmStats)], c.c_int),
        "yk_film_save": ([c.c_char_p, P(RenderParams), c.c_uint64, c.c_uint32, c.c_void_p, c.c_void_p],
                         c.c_int),
        "yk_film_load": ([c.c_char_p, P(RenderParams), P(c.c_uint64), P(c.c_uint32), c.c_void_p,
                          c.c_void_p, c.c_uint64], c.c_int),
        "yk_scene_hash": ([P(Sphere), c.c_uint32, P(Camera)], c.c_uint64),
        "ykgpu_film_accumulate_adaptive": ([c.c_void_p, c.c_double, c.c_uint32, P(FilmPass)], c.c_int),
        "ykgpu_film_counts": ([c.c_void_p, c.c_void_p, P(c.c_uint32), P(c.c_uint32)], c.c_int),
        "ykgpu_film_write_counts": ([c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p], c.c_int),
        "yk_film_save_counts": ([c.c_char_p, P(RenderParams), c.c_uint64, c.c_void_p, c.c_void_p, c.c_void_p],
                                c.c_int),
        "yk_film_load_counts": ([c.c_char_p, P(RenderParams), P(c.c_uint64), c.c_void_p, c.c_void_p,
                                 c.c_void_p, c.c_uint64], c.c_int),
        "yk_denoise_defaults": ([P(DenoiseParams)], c.c_int),
        "ykgpu_film_denoise": ([c.c_void_p, P(DenoiseParams), c.c_void_p, c.c_void_p, P(DenoiseStats)], c.c_int),
        "yk_guided_defaults": ([P(DenoiseParams), P(FeatureParams)], c.c_int),
        "ykgpu_film_features": ([c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p, P(c.c_double)], c.c_int),
        "ykgpu_film_denoise_guided": ([c.c_void_p, P(DenoiseParams), P(FeatureParams), c.c_void_p, c.c_void_p,
                                       P(GuidedStats)], c.c_int),
        "yk_guided_sampled_defaults": ([P(DenoiseParams), P(FeatureParams), P(c.c_uint32)], c.c_int),
        "ykgpu_film_features_sampled": ([c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p, P(SampledFeaturesStats)],
                                        c.c_int),
        "ykgpu_film_denoise_guided_sampled": ([c.c_void_p, P(DenoiseParams), P(FeatureParams), c.c_uint32, c.c_void_p,
                                               c.c_void_p, P(GuidedStats)], c.c_int),
        "ykgpu_film_mattes": ([c.c_void_p, c.c_uint32, c.c_void_p, P(MatteStats)], c.c_int),
        "ykgpu_film_matte_coverage": ([c.c_void_p, c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p, P(MatteCoverageStats)],
                                      c.c_int),
        "ykgpu_cast_rays": ([c.c_void_p, c.c_void_p, c.c_uint64, c.c_uint32, c.c_void_p], c.c_int),
        "ykgpu_cast_rays_async": ([c.c_void_p, c.c_void_p, c.c_uint64, c.c_uint32, c.c_void_p, c.c_void_p], c.c_int),
        "ykgpu_cast_get_stats": ([c.c_void_p, P(CastStats)], c.c_int),
        "ykgpu_radiance_rays": ([c.c_void_p, P(RadianceParams), c.c_void_p, c.c_uint64, c.c_void_p], c.c_int),
        "ykgpu_radiance_rays_async": ([c.c_void_p, P(RadianceParams), c.c_void_p, c.c_uint64, c.c_void_p, c.c_void_p],
                                      c.c_int),
        "ykgpu_radiance_get_stats": ([c.c_void_p, P(RadianceStats)], c.c_int),
        "yk_camera_sample_ray": ([P(Camera), P(RenderParams), c.c_uint32, c.c_uint32, c.c_uint32, c.c_void_p], c.c_int),
        "yk_camera_sample_rays": ([P(Camera), P(RenderParams), c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint64,
                                   c.c_void_p], c.c_int),
        "ykgpu_gather_points": ([c.c_void_p, P(GatherParams), c.c_void_p, c.c_uint64, c.c_void_p], c.c_int),
        "ykgpu_gather_points_async": ([c.c_void_p, P(GatherParams), c.c_void_p, c.c_uint64, c.c_void_p, c.c_void_p],
                                      c.c_int),
        "ykgpu_gather_get_stats": ([c.c_void_p, P(GatherStats)], c.c_int),
        "yk_gather_sample_ray": ([c.c_void_p, c.c_uint32, c.c_uint32, c.c_void_p], c.c_int),
        "yk_gather_sample_rays": ([c.c_void_p, c.c_uint64, c.c_uint32, c.c_uint32, c.c_void_p], c.c_int),
    }
    # the group film calls take the film calls' arguments (include/ykgpu.h "group films"); the two
    # filters report yk_group_denoise_stats
    for name in ("create", "destroy", "params", "accumulate", "accumulate_adaptive", "resolve", "read", "write",
                 "counts", "write_counts", "error", "features", "denoise", "denoise_guided", "features_sampled",
                 "denoise_guided_sampled", "mattes", "matte_coverage"):
        args, res = sig["ykgpu_film_" + name]
        if name.startswith("denoise"):
            args = args[:-1] + [P(GroupDenoiseStats)]
        sig["ykgpu_group_film_" + name] = (args, res)
    for name, (args, res) in sig.items():
        f = getattr(lib, name)
        f.argtypes, f.restype = args, res
    # (a test hook, not part of the C-ABI: _feature_lazy_words below)
    lib.yk_features_sampled_lazy_words.argtypes, lib.yk_features_sampled_lazy_words.restype = [c.c_uint32], None
    # (likewise: the seed table's switches, Renderer.__init__, and its test hook; a library of an
    # earlier revision, which the A/B tools load through YKGPU_LIB_OVERRIDE, has neither)
    if hasattr(lib, "yk_seed_table_configure"):
        lib.yk_seed_table_configure.argtypes, lib.yk_seed_table_configure.restype = [c.c_void_p, c.c_int, c.c_uint64], None
        lib.yk_seed_table_test.argtypes, lib.yk_seed_table_test.restype = [c.c_uint32], None
    if lib.ykgpu_abi_version() != ABI_VERSION:
        raise YkError("ABI version mismatch")
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        msg = load_library().ykgpu_last_error().decode(errors="replace")
        raise YkError(f"{records.ERRORS.get(rc, rc)}: {msg}")


def device_count() -> int:
    n = ctypes.c_int(0)
    rc = load_library().ykgpu_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


def reference_camera() -> Camera:
    cam = Camera()
    _check(load_library().yk_camera_reference(ctypes.byref(cam)))
    return cam


def build_scene(name: str, seed: int = 0):
    """Named scenes of include/ykgpu.h (host only).  Returns (spheres ctypes array, Camera)."""
    lib = load_library()
    n, cam = ctypes.c_uint32(0), Camera()
    _check(lib.yk_scene_build(name.encode(), seed, None, 0, ctypes.byref(n), ctypes.byref(cam)))
    arr = (Sphere * n.value)()
    _check(lib.yk_scene_build(name.encode(), seed, arr, n.value, ctypes.byref(n), None))
    return arr, cam


def write_scene(path: str, spheres, camera: Camera):
    """Scene file (include/ykgpu.h yk_scene_write): tuple order, exact doubles."""
    arr = spheres if isinstance(spheres, ctypes.Array) else sphere_array(spheres)
    _check(load_library().yk_scene_write(os.fsencode(path), arr, len(arr), ctypes.byref(camera)))


def read_scene(path: str):
    """Returns (spheres ctypes array, Camera) from a scene file."""
    lib = load_library()
    n, cam = ctypes.c_uint32(0), Camera()
    _check(lib.yk_scene_read(os.fsencode(path), None, 0, ctypes.byref(n), ctypes.byref(cam)))
    arr = (Sphere * n.value)()
    _check(lib.yk_scene_read(os.fsencode(path), arr, n.value, ctypes.byref(n), None))
    return arr, cam


def scene_hash(spheres, camera: Camera) -> int:
    """yk_scene_hash: the scene a saved film belongs to (host only)."""
    arr = spheres if isinstance(spheres, ctypes.Array) else sphere_array(spheres)
    return load_library().yk_scene_hash(arr, len(arr), ctypes.byref(camera))


def save_film(path: str, params: RenderParams, scene: int, done: int, sums, sumsq):
    """yk_film_save (host only): params, scene hash, done and the raw doubles of a film state."""
    a = np.ascontiguousarray(sums, dtype=np.float64)
    b = np.ascontiguousarray(sumsq, dtype=np.float64)
    n = params.row_count * params.tile_width() * 3
    if a.size != n or b.size != n:
        raise YkError("save_film: sums and sumsq must hold row_count * tile width * 3 doubles")
    rc = load_library().yk_film_save(os.fsencode(path), ctypes.byref(params), scene, done,
                                     a.ctypes.data, b.ctypes.data)
    if rc != 0:
        raise YkError(f"{records.ERRORS.get(rc, rc)}: cannot save the film to {path}")


def load_film(path: str):
    """yk_film_load (host only).  Returns (RenderParams, scene hash, done, sums, sumsq), the arrays
    float64[row_count, tile width, 3]."""
    lib = load_library()
    p, h, done = RenderParams(), ctypes.c_uint64(0), ctypes.c_uint32(0)
    rc = lib.yk_film_load(os.fsencode(path), ctypes.byref(p), ctypes.byref(h), ctypes.byref(done),
                          None, None, 0)
    if rc == 0:
        shape = (p.row_count, p.tile_width(), 3)
        sums, sumsq = np.empty(shape, np.float64), np.empty(shape, np.float64)
        rc = lib.yk_film_load(os.fsencode(path), ctypes.byref(p), ctypes.byref(h), ctypes.byref(done),
                              sums.ctypes.data, sumsq.ctypes.data, shape[0] * shape[1])
    if rc != 0:
        raise YkError(f"{records.ERRORS.get(rc, rc)}: {path} is not a readable film file")
    return p, h.value, done.value, sums, sumsq


def save_film_counts(path: str, params: RenderParams, scene: int, counts, sums, sumsq):
    """yk_film_save_counts (host only): a v2 film file, with a sample count per pixel."""
    n = params.row_count * params.tile_width()
    k = np.ascontiguousarray(counts, dtype=np.uint32)
    a = np.ascontiguousarray(sums, dtype=np.float64)
    b = np.ascontiguousarray(sumsq, dtype=np.float64)
    if k.size != n or a.size != 3 * n or b.size != 3 * n:
        raise YkError("save_film_counts: counts must hold row_count * tile width words, sums and sumsq 3 doubles each")
    rc = load_library().yk_film_save_counts(os.fsencode(path), ctypes.byref(params), scene, k.ctypes.data,
                                            a.ctypes.data, b.ctypes.data)
    if rc != 0:
        raise YkError(f"{records.ERRORS.get(rc, rc)}: cannot save the film to {path}")


def load_film_counts(path: str):
    """yk_film_load_counts (host only): a v2 film file, or a v1 file with every count equal to its
    done.  Returns (RenderParams, scene hash, counts uint32[row_count, tile width], sums, sumsq)."""
    lib = load_library()
    p, h = RenderParams(), ctypes.c_uint64(0)
    rc = lib.yk_film_load_counts(os.fsencode(path), ctypes.byref(p), ctypes.byref(h), None, None, None, 0)
    if rc == 0:
        shape = (p.row_count, p.tile_width())
        counts = np.empty(shape, np.uint32)
        sums, sumsq = np.empty(shape + (3,), np.float64), np.empty(shape + (3,), np.float64)
        rc = lib.yk_film_load_counts(os.fsencode(path), ctypes.byref(p), ctypes.byref(h), counts.ctypes.data,
                                     sums.ctypes.data, sumsq.ctypes.data, shape[0] * shape[1])
    if rc != 0:
        raise YkError(f"{records.ERRORS.get(rc, rc)}: {path} is not a readable film file")
    return p, h.value, counts, sums, sumsq


def denoise_defaults() -> DenoiseParams:
    """yk_denoise_defaults (host only): radius 5, patch 1, k2 0.5, alpha 1.0, eps 1e-10."""
    dp = DenoiseParams()
    _check(load_library().yk_denoise_defaults(ctypes.byref(dp)))
    return dp


def guided_defaults():
    """yk_guided_defaults (host only): the (DenoiseParams, FeatureParams) pair tuned together
    (DESIGN.md §6.4)."""
    dp, fp = DenoiseParams(), FeatureParams()
    _check(load_library().yk_guided_defaults(ctypes.byref(dp), ctypes.byref(fp)))
    return dp, fp


def guided_sampled_defaults():
    """yk_guided_sampled_defaults (host only): the (DenoiseParams, FeatureParams, n_samples) point
    chosen for the sampled feature pass."""
    dp, fp, n = DenoiseParams(), FeatureParams(), ctypes.c_uint32(0)
    _check(load_library().yk_guided_sampled_defaults(ctypes.byref(dp), ctypes.byref(fp), ctypes.byref(n)))
    return dp, fp, n.value


class _feature_lazy_words:
    """YKGPU_FEATURE_LAZY_WORDS, read at each sampled feature call: the mt19937
    words a sample's start may draw before the sampled pass hands its pixel to the whole-engine
    redo, clamped to 4..227.  A diagnostic for tests (the planes do not depend on it); the package
    reads it, not the library, and hands it over for the one call."""

    def __init__(self, lib):
        self._lib = lib
        v = os.environ.get("YKGPU_FEATURE_LAZY_WORDS")
        try:
            self._words = min(227, max(4, int(v))) if v else 0
        except ValueError:
            self._words = 0

    def __enter__(self):
        if self._words:
            self._lib.yk_features_sampled_lazy_words(self._words)

    def __exit__(self, *exc):
        if self._words:
            self._lib.yk_features_sampled_lazy_words(0)


def camera_sample_rays(camera: Camera, params: RenderParams, ys, xs, ss) -> np.ndarray:
    """yk_camera_sample_ray (host only) over arrays: records.PATH_RAY_DTYPE[N], the ray, seed and skip
    with which render() enters ray_color for sample ss[i] of pixel (ys[i], xs[i]) of the image
    `params` names.  Renderer.radiance on a pixel's samples, added up in sample order, is that pixel
    of Renderer.render_sums."""
    lib = load_library()
    ys, xs, ss = np.broadcast_arrays(np.asarray(ys, np.int64), np.asarray(xs, np.int64), np.asarray(ss, np.int64))
    if ys.size and (min(ys.min(), xs.min(), ss.min()) < 0 or max(ys.max(), xs.max(), ss.max()) > 0xFFFFFFFF):
        raise YkError("camera_sample_rays: indices must fit uint32")
    ys, xs, ss = (np.ascontiguousarray(a.ravel(), dtype=np.uint32) for a in (ys, xs, ss))
    out = np.zeros(ys.size, records.PATH_RAY_DTYPE)
    rc = lib.yk_camera_sample_rays(ctypes.byref(camera), ctypes.byref(params), ys.ctypes.data, xs.ctypes.data,
                                   ss.ctypes.data, ys.size, out.ctypes.data)
    if rc != 0:
        raise YkError(f"{records.ERRORS.get(rc, rc)}: camera_sample_rays: a sample outside the image, or fp32")
    return out


def gather_points(points, normals, seeds, skip=0) -> np.ndarray:
    """records.GATHER_POINT_DTYPE[N] from points and normals float64[N, 3] and seeds and skip, scalars
    or uint32[N]."""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
    if p.shape != n.shape:
        raise YkError("gather: points and normals must both be [N, 3]")
    pts = np.zeros(p.shape[0], records.GATHER_POINT_DTYPE)
    pts["p"], pts["n"] = p, n
    pts["seed"] = np.broadcast_to(np.asarray(seeds, np.uint32), (len(pts),))
    pts["skip"] = np.broadcast_to(np.asarray(skip, np.uint32), (len(pts),))
    return pts


def gather_sample_rays(points, n_samples: int, rng=records.RNG_MT19937) -> np.ndarray:
    """yk_gather_sample_rays (host only): records.PATH_RAY_DTYPE[N, n_samples], the path ray of every
    sample of records.GATHER_POINT_DTYPE[N] points.  Renderer.radiance_rays on a point's rays, folded
    in sample order, is that point's record of Renderer.gather_points."""
    pts = np.ascontiguousarray(points, dtype=records.GATHER_POINT_DTYPE).reshape(-1)
    if n_samples < 1 or n_samples > records.GATHER_MAX_SAMPLES:
        raise YkError("gather_sample_rays: n_samples must be 1..65536")
    out = np.zeros((pts.size, n_samples), records.PATH_RAY_DTYPE)
    rc = load_library().yk_gather_sample_rays(pts.ctypes.data if pts.size else None, pts.size, rng, n_samples,
                                              out.ctypes.data if pts.size else None)
    if rc != 0:
        raise YkError(f"{records.ERRORS.get(rc, rc)}: gather_sample_rays: an unknown rng")
    return out


class Film:
    """A progressive film (ykgpu_film, include/ykgpu.h): the resumable accumulation state of one
    tile.  Made by Renderer.film(params); any chunking of the samples yields the one-shot render's
    sums and image bit for bit."""

    _PREFIX = "ykgpu_film_"  # (GroupFilm: the same calls on a group)
    _DENOISE_STATS, _GUIDED_STATS = DenoiseStats, GuidedStats

    def __init__(self, renderer: "Renderer", params: RenderParams):
        self._lib = renderer._lib
        self._ren = renderer
        self._f = ctypes.c_void_p()
        _check(self._fn("create")(self._owner_handle(renderer), ctypes.byref(params), ctypes.byref(self._f)))
        self.params = RenderParams()
        _check(self._fn("params")(self._f, ctypes.byref(self.params)))
        self._shape = (self.params.row_count, self.params.tile_width())
        renderer._films.add(self)

    def _fn(self, name):
        return getattr(self._lib, self._PREFIX + name)

    @staticmethod
    def _owner_handle(owner):
        return owner._ctx

    def close(self):
        if self._f:
            self._fn("destroy")(self._f)
            self._f = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def target(self) -> int:
        return self.params.samples_per_pixel

    @property
    def done(self) -> int:
        n = ctypes.c_uint32(0)
        _check(self._fn("read")(self._f, None, None, ctypes.byref(n)))
        return n.value

    def accumulate(self, n_samples: int) -> int:
        """Renders samples [done, done + n_samples) into the film; returns the new done."""
        _check(self._fn("accumulate")(self._f, n_samples))
        return self.done

    def accumulate_adaptive(self, threshold2: float, n_samples: int) -> FilmPass:
        """One adaptive pass (ykgpu_film_accumulate_adaptive): up to n_samples more samples for every
        pixel below the target that has fewer than two samples or e2 > threshold2."""
        out = FilmPass()
        _check(self._fn("accumulate_adaptive")(self._f, threshold2, n_samples, ctypes.byref(out)))
        return out

    def counts(self) -> np.ndarray:
        """uint32[row_count, tile width]: the samples each pixel holds."""
        out = np.empty(self._shape, np.uint32)
        _check(self._fn("counts")(self._f, out.ctypes.data, None, None))
        return out

    def count_range(self):
        """(min, max) of counts(), without reading the map."""
        lo, hi = ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check(self._fn("counts")(self._f, None, ctypes.byref(lo), ctypes.byref(hi)))
        return lo.value, hi.value

    def write_counts(self, sums, sumsq, counts):
        """Restores a state with a count per pixel."""
        a = np.ascontiguousarray(sums, dtype=np.float64)
        b = np.ascontiguousarray(sumsq, dtype=np.float64)
        k = np.ascontiguousarray(counts, dtype=np.uint32)
        if a.shape != self._shape + (3,) or b.shape != self._shape + (3,) or k.shape != self._shape:
            raise YkError(f"Film.write_counts: sums and sumsq must have shape {self._shape + (3,)}, counts {self._shape}")
        _check(self._fn("write_counts")(self._f, a.ctypes.data, b.ctypes.data, k.ctypes.data))

    def resolve(self) -> np.ndarray:
        """uint8[row_count, tile width, 3]: to_color3b of the sums at the divisor done (each
        pixel's own count once they differ)."""
        out = np.empty(self._shape + (3,), np.uint8)
        _check(self._fn("resolve")(self._f, out.ctypes.data))
        return out

    def read(self):
        """(sums, sumsq, done): float64[row_count, tile width, 3] each."""
        sums, sumsq = np.empty(self._shape + (3,), np.float64), np.empty(self._shape + (3,), np.float64)
        n = ctypes.c_uint32(0)
        _check(self._fn("read")(self._f, sums.ctypes.data, sumsq.ctypes.data, ctypes.byref(n)))
        return sums, sumsq, n.value

    def write(self, sums, sumsq, done: int):
        """Restores a state read earlier."""
        a = np.ascontiguousarray(sums, dtype=np.float64)
        b = np.ascontiguousarray(sumsq, dtype=np.float64)
        if a.shape != self._shape + (3,) or b.shape != self._shape + (3,):
            raise YkError(f"Film.write: sums and sumsq must have shape {self._shape + (3,)}")
        _check(self._fn("write")(self._f, a.ctypes.data, b.ctypes.data, done))

    def error(self, threshold2: float = 0.0, want_map: bool = True):
        """(e2 float64[row_count, tile width] | None, stats dict): the squared standard error of
        each pixel's mean, worst channel, and the pixels with e2 > threshold2."""
        e2 = np.empty(self._shape, np.float64) if want_map else None
        st = FilmStats()
        _check(self._fn("error")(self._f, threshold2, e2.ctypes.data if want_map else None,
                                          ctypes.byref(st)))
        return e2, st.as_dict()

    def denoise(self, radius: int = 5, patch: int = 1, k2: float = 0.5, alpha: float = 1.0, eps: float = 1e-10,
                want_mean: bool = True, want_rgb: bool = True):
        """(mean float64[row_count, tile width, 3] | None, rgb uint8[row_count, tile width, 3] | None,
        stats dict): the variance-guided non-local-means filter of include/ykgpu.h "film denoise" on
        the film's tile.  Reads the film only; every pixel needs at least two samples."""
        mean = np.empty(self._shape + (3,), np.float64) if want_mean else None
        rgb = np.empty(self._shape + (3,), np.uint8) if want_rgb else None
        dp, st = DenoiseParams(radius, patch, k2, alpha, eps), self._DENOISE_STATS()
        _check(self._fn("denoise")(self._f, ctypes.byref(dp), mean.ctypes.data if want_mean else None,
                                            rgb.ctypes.data if want_rgb else None, ctypes.byref(st)))
        return mean, rgb, st.as_dict()

    def features(self, grid: int = 2):
        """(mean float64[row_count, tile width, 7], var float64[row_count, tile width, 7], ms): the
        first-hit albedo (0..2), normal (3..5) and depth (6) of include/ykgpu.h "film features" on
        the film's tile, and the variances of those means over the grid x grid sub-rays.  Computed
        once per (film, grid): ms is 0 when the film's cached pass was reused."""
        mean = np.empty(self._shape + (7,), np.float64)
        var = np.empty(self._shape + (7,), np.float64)
        ms = ctypes.c_double(0.0)
        _check(self._fn("features")(self._f, grid, mean.ctypes.data, var.ctypes.data, ctypes.byref(ms)))
        return mean, var, ms.value

    def denoise_guided(self, colour: DenoiseParams = None, feat: FeatureParams = None, want_mean: bool = True,
                       want_rgb: bool = True):
        """(mean | None, rgb | None, stats dict) like denoise(): the filter of include/ykgpu.h "film
        features", its weight bounded by the feature planes' distance.  colour / feat None: that side
        of guided_defaults()."""
        mean = np.empty(self._shape + (3,), np.float64) if want_mean else None
        rgb = np.empty(self._shape + (3,), np.uint8) if want_rgb else None
        st = self._GUIDED_STATS()
        _check(self._fn("denoise_guided")(
            self._f, ctypes.byref(colour) if colour is not None else None,
            ctypes.byref(feat) if feat is not None else None, mean.ctypes.data if want_mean else None,
            rgb.ctypes.data if want_rgb else None, ctypes.byref(st)))
        return mean, rgb, st.as_dict()

    def features_sampled(self, n_samples: int):
        """(mean float64[row_count, tile width, 7], var likewise, stats dict): the feature planes of
        include/ykgpu.h "sampled film features", from the first hits of the film's own first
        n_samples samples (lens and jitter included).  Computed once per (film, n_samples): ms is 0
        when the film's cached pass was reused."""
        mean = np.empty(self._shape + (7,), np.float64)
        var = np.empty(self._shape + (7,), np.float64)
        st = SampledFeaturesStats()
        with _feature_lazy_words(self._lib):
            _check(self._fn("features_sampled")(self._f, n_samples, mean.ctypes.data, var.ctypes.data, ctypes.byref(st)))
        return mean, var, st.as_dict()

    def denoise_guided_sampled(self, colour: DenoiseParams = None, feat: FeatureParams = None, n_samples: int = None,
                               want_mean: bool = True, want_rgb: bool = True):
        """denoise_guided() with the sampled feature planes of the film's first n_samples samples as
        guides (feat.grid is ignored).  colour / feat / n_samples None: that part of
        guided_sampled_defaults()."""
        mean = np.empty(self._shape + (3,), np.float64) if want_mean else None
        rgb = np.empty(self._shape + (3,), np.uint8) if want_rgb else None
        st = self._GUIDED_STATS()
        if n_samples is None:
            n_samples = guided_sampled_defaults()[2]
        with _feature_lazy_words(self._lib):
            _check(self._fn("denoise_guided_sampled")(
                self._f, ctypes.byref(colour) if colour is not None else None,
                ctypes.byref(feat) if feat is not None else None, n_samples, mean.ctypes.data if want_mean else None,
                rgb.ctypes.data if want_rgb else None, ctypes.byref(st)))
        return mean, rgb, st.as_dict()

    def mattes(self, n_samples: int = 0):
        """(table records.MATTE_DTYPE[row_count, tile width], stats dict): the id-coverage table of
        include/ykgpu.h "film mattes": per pixel, the spheres the first hits of its samples landed
        on and how many samples each got.  n_samples 0: every pixel's own count in the film; else the
        first n_samples samples (computed once per (film, n_samples): ms is 0 when the film's table
        was reused)."""
        table = np.zeros(self._shape, records.MATTE_DTYPE)
        st = MatteStats()
        with _feature_lazy_words(self._lib):
            _check(self._fn("mattes")(self._f, n_samples, table.ctypes.data, ctypes.byref(st)))
        return table, st.as_dict()

    def matte_coverage(self, ids, want_cov: bool = True, want_grey: bool = True):
        """(cov float64[row_count, tile width] | None, grey uint8[row_count, tile width] | None, stats
        dict): the share of each pixel's samples whose first hit is one of `ids` (sphere indices
        and/or records.MATTE_SKY), from the table the last mattes() call left in the film; grey is
        trunc(clamp(cov, 0, 0.999) * 256).  A lower bound where the pixel's `other` is not 0."""
        k = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        cov = np.empty(self._shape, np.float64) if want_cov else None
        grey = np.empty(self._shape, np.uint8) if want_grey else None
        st = MatteCoverageStats()
        _check(self._fn("matte_coverage")(self._f, k.ctypes.data if k.size else None, k.size,
                                          cov.ctypes.data if want_cov else None, grey.ctypes.data if want_grey else None,
                                          ctypes.byref(st)))
        return cov, grey, st.as_dict()

    def render_until(self, threshold: float, chunk: int) -> dict:
        """Accumulates `chunk` samples at a time until no pixel's standard error exceeds
        `threshold` (e2 <= threshold**2 everywhere) or the target is reached; returns the stats
        of the last error map."""
        if chunk < 1:
            raise YkError("render_until: chunk must be >= 1")
        while True:
            done = self.done
            if done >= 2:
                _, st = self.error(threshold * threshold, want_map=False)
                if st["pixels_over"] == 0 or done >= self.target:
                    return st
            elif done >= self.target:  # a target of one sample has no error estimate
                return FilmStats(self._shape[0] * self._shape[1], 0, 0.0, done, self.target).as_dict()
            self.accumulate(min(chunk, self.target - done))

    def save(self, path: str, scene: int):
        """Checkpoint: the film's params, `scene` (scene_hash of the scene it renders) and state."""
        sums, sumsq, done = self.read()
        lo, hi = self.count_range()
        if lo != hi:  # (a v2 file only when it is needed: uniform films stay readable by yk_film_load)
            save_film_counts(path, self.params, scene, self.counts(), sums, sumsq)
        else:
            save_film(path, self.params, scene, done, sums, sumsq)

    def load(self, path: str, scene: int) -> int:
        """Resume: restores the state saved in `path`; refuses a file whose params or scene hash
        differ from the film's.  Returns done (the smallest count)."""
        p, h, counts, sums, sumsq = load_film_counts(path)
        if bytes(p) != bytes(self.params):
            raise YkError(f"{path} was saved with other render params than this film's")
        if h != scene:
            raise YkError(f"{path} was saved for another scene")
        if counts.min() == counts.max():
            self.write(sums, sumsq, int(counts.min()))
        else:
            self.write_counts(sums, sumsq, counts)
        return int(counts.min())


class GroupFilm(Film):
    """A group film (ykgpu_group_film, include/ykgpu.h "group films"): Film's methods and Film's bytes,
    with the sample chunks and the filters' work spread over the entries of a Group.  Made by
    Group.film(params).  The filters' stats are GroupDenoiseStats (exchange_ms beside the others)."""
    _PREFIX = "ykgpu_group_film_"
    _DENOISE_STATS = _GUIDED_STATS = GroupDenoiseStats

    @staticmethod
    def _owner_handle(owner):
        return owner._g


class Renderer:
    """One device context (ykgpu_context): owns the scene in HBM, scratch and a stream."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        self._ctx = ctypes.c_void_p()
        self._films = weakref.WeakSet()
        _check(self._lib.ykgpu_context_create(device, ctypes.byref(self._ctx)))
        self.device = device
        # the seed table's switches, read here, when the context is created: the
        # package reads them, not the library, and hands them over through a hook outside the C-ABI
        off = os.environ.get("YKGPU_SEED_TABLE", "").strip() == "0"
        cap = os.environ.get("YKGPU_SEED_TABLE_MAX_MB")
        if (off or cap is not None) and hasattr(self._lib, "yk_seed_table_configure"):
            try:
                max_bytes = min(max(int(cap), 0), 1 << 40) << 20 if cap is not None else 8 << 30
            except ValueError:
                max_bytes = 8 << 30  # (the library's default cap)
            self._lib.yk_seed_table_configure(self._ctx, 0 if off else 1, max_bytes)

    def film(self, params: RenderParams) -> Film:
        """A progressive film of the tile `params` names (include/ykgpu.h)."""
        return Film(self, params)

    def close(self):
        for f in list(self._films):  # films go before their context
            f.close()
        if self._ctx:
            self._lib.ykgpu_context_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_scene(self, spheres, camera: Camera):
        arr = spheres if isinstance(spheres, ctypes.Array) else sphere_array(spheres)
        _check(self._lib.ykgpu_set_scene(self._ctx, arr, len(arr), ctypes.byref(camera)))

    def render(self, params: RenderParams) -> np.ndarray:
        """Host RGB8 image of the tile: uint8[row_count, W, 3] (image_t layout)."""
        out = np.empty((params.row_count, params.tile_width(), 3), np.uint8)
        _check(self._lib.ykgpu_render(self._ctx, ctypes.byref(params), out.ctypes.data))
        return out

    def render_sums(self, params: RenderParams) -> np.ndarray:
        out = np.empty((params.row_count, params.tile_width(), 3), np.float64)
        _check(self._lib.ykgpu_render_sums(self._ctx, ctypes.byref(params), out.ctypes.data))
        return out

    def render_trace(self, params: RenderParams, max_rays: int):
        """ray_color's rays (verbose level 3, raytracer.hpp:21-25) of every sample of the tile:
        (rays float64[row_count, W, spp, max_rays, 6], counts uint32[row_count, W, spp])."""
        shape = (params.row_count, params.tile_width(), params.samples_per_pixel)
        rays = np.zeros(shape + (max_rays, 6), np.float64)
        counts = np.zeros(shape, np.uint32)
        _check(self._lib.ykgpu_render_trace(self._ctx, ctypes.byref(params), max_rays, rays.ctypes.data,
                                            counts.ctypes.data))
        return rays, counts

    def render_async(self, params: RenderParams, rgb_device_ptr: int, stream_ptr: int = 0):
        """Enqueue into device memory (e.g. a torch.uint8 CUDA tensor's data_ptr())."""
        _check(self._lib.ykgpu_render_async(self._ctx, ctypes.byref(params),
                                            ctypes.c_void_p(rgb_device_ptr),
                                            ctypes.c_void_p(stream_ptr or None)))

    def math_sqrt(self, values) -> np.ndarray:
        """The device's math::sqrt (math.hpp:10-19) on a float64 array (diagnostic)."""
        a = np.ascontiguousarray(values, dtype=np.float64)
        out = np.empty_like(a)
        _check(self._lib.ykgpu_math_sqrt(self._ctx, a.ctypes.data, out.ctypes.data, a.size))
        return out

    def math_sqrt_f32(self, values) -> np.ndarray:
        """The FP32 path's math::sqrt<float> on a float32 array (diagnostic)."""
        a = np.ascontiguousarray(values, dtype=np.float32)
        out = np.empty_like(a)
        _check(self._lib.ykgpu_math_sqrt_f32(self._ctx, a.ctypes.data, out.ctypes.data, a.size))
        return out

    def math_div(self, num3, den) -> np.ndarray:
        """The renderer's vector / scalar division: num3[i, k] / den[i] (diagnostic)."""
        a = np.ascontiguousarray(num3, dtype=np.float64).reshape(-1, 3)
        b = np.ascontiguousarray(den, dtype=np.float64).reshape(-1)
        assert a.shape[0] == b.shape[0]
        out = np.empty_like(a)
        _check(self._lib.ykgpu_math_div(self._ctx, a.ctypes.data, b.ctypes.data, out.ctypes.data, b.size))
        return out

    def math_div_f32(self, num3, den) -> np.ndarray:
        """The FP32 path's vector / scalar division: num3[i, k] / den[i] in float (diagnostic)."""
        a = np.ascontiguousarray(num3, dtype=np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(den, dtype=np.float32).reshape(-1)
        assert a.shape[0] == b.shape[0]
        out = np.empty_like(a)
        _check(self._lib.ykgpu_math_div_f32(self._ctx, a.ctypes.data, b.ctypes.data, out.ctypes.data, b.size))
        return out

    def stats(self) -> dict:
        st = RenderStats()
        _check(self._lib.ykgpu_get_stats(self._ctx, ctypes.byref(st)))
        return st.as_dict()

    def cast_rays(self, origins, directions, t_min=records.T_MIN, t_max=float("inf"), any_hit: bool = False,
                  linear_scan: bool = False, count_work: bool = False) -> np.ndarray:
        """The reference's world.hit for N rays (include/ykgpu.h "ray queries"): origins and
        directions float64[N, 3], the limits scalars or float64[N].  Returns records.HIT_DTYPE[N]:
        p, normal, t, id (records.NO_HIT_ID when none) and flags (records.HIT_*)."""
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
        if o.shape != d.shape:
            raise YkError("cast_rays: origins and directions must both be [N, 3]")
        n = o.shape[0]
        rays = np.empty(n, records.RAY_DTYPE)
        rays["origin"], rays["direction"] = o, d
        rays["t_min"] = np.broadcast_to(np.asarray(t_min, np.float64), (n,))
        rays["t_max"] = np.broadcast_to(np.asarray(t_max, np.float64), (n,))
        hits = np.empty(n, records.HIT_DTYPE)
        flags = ((records.CAST_ANY_HIT if any_hit else 0) | (records.CAST_LINEAR_SCAN if linear_scan else 0) |
                 (records.CAST_COUNT_WORK if count_work else 0))
        _check(self._lib.ykgpu_cast_rays(self._ctx, rays.ctypes.data if n else None, n, flags,
                                         hits.ctypes.data if n else None))
        return hits

    def cast_rays_device(self, rays_ptr: int, n: int, hits_ptr: int, stream_ptr: int = 0, flags: int = 0):
        """Enqueue a cast over device memory (ykgpu_cast_rays_async): n yk_ray records at rays_ptr,
        n yk_hit records written at hits_ptr (e.g. float64 [N, 8] CUDA tensors' data_ptr()), on the
        stream (0: the context's).  Does not synchronise."""
        _check(self._lib.ykgpu_cast_rays_async(self._ctx, ctypes.c_void_p(rays_ptr or None), n, flags,
                                               ctypes.c_void_p(hits_ptr or None),
                                               ctypes.c_void_p(stream_ptr or None)))

    def cast_stats(self) -> dict:
        """yk_cast_stats of the last synchronous cast_rays."""
        st = CastStats()
        _check(self._lib.ykgpu_cast_get_stats(self._ctx, ctypes.byref(st)))
        return st.as_dict()

    @staticmethod
    def _radiance_params(max_depth, t_min, rng, linear_scan, count_work) -> RadianceParams:
        flags = (records.RADIANCE_LINEAR_SCAN if linear_scan else 0) | (records.RADIANCE_COUNT_WORK if count_work else 0)
        return RadianceParams(max_depth, rng, flags, 0, t_min, 0)

    def radiance(self, origins, directions, seeds, skip=0, max_depth=50, t_min=records.T_MIN,
                 rng=records.RNG_MT19937, linear_scan: bool = False, count_work: bool = False) -> np.ndarray:
        """The reference's ray_color for N rays (include/ykgpu.h "radiance queries"): origins and
        directions float64[N, 3], seeds and skip scalars or uint32[N] (the path's engine is
        Engine(seed) with skip words discarded).  Returns records.RADIANCE_DTYPE[N]: colour, t_first,
        id_first, id_last, words, segments and flags (records.RAD_*)."""
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
        if o.shape != d.shape:
            raise YkError("radiance: origins and directions must both be [N, 3]")
        rays = np.zeros(o.shape[0], records.PATH_RAY_DTYPE)
        rays["origin"], rays["direction"] = o, d
        rays["seed"] = np.broadcast_to(np.asarray(seeds, np.uint32), (len(rays),))
        rays["skip"] = np.broadcast_to(np.asarray(skip, np.uint32), (len(rays),))
        return self.radiance_rays(rays, max_depth, t_min, rng, linear_scan, count_work)

    def radiance_rays(self, rays, max_depth=50, t_min=records.T_MIN, rng=records.RNG_MT19937,
                      linear_scan: bool = False, count_work: bool = False) -> np.ndarray:
        """radiance() on records.PATH_RAY_DTYPE[N] (camera_sample_rays' output, for one)."""
        rays = np.ascontiguousarray(rays, dtype=records.PATH_RAY_DTYPE)
        n = rays.size
        out = np.zeros(n, records.RADIANCE_DTYPE)
        par = self._radiance_params(max_depth, t_min, rng, linear_scan, count_work)
        _check(self._lib.ykgpu_radiance_rays(self._ctx, ctypes.byref(par), rays.ctypes.data if n else None, n,
                                             out.ctypes.data if n else None))
        return out

    def radiance_device(self, rays_ptr: int, n: int, out_ptr: int, max_depth=50, t_min=records.T_MIN,
                        rng=records.RNG_MT19937, linear_scan: bool = False, count_work: bool = False,
                        stream_ptr: int = 0):
        """Enqueue a radiance query over device memory (ykgpu_radiance_rays_async): n yk_path_ray
        records at rays_ptr, n yk_radiance records written at out_ptr (e.g. [N, 64] uint8 or [N, 8]
        float64 CUDA tensors' data_ptr()), on the stream (0: the context's).  Does not synchronise."""
        par = self._radiance_params(max_depth, t_min, rng, linear_scan, count_work)
        _check(self._lib.ykgpu_radiance_rays_async(self._ctx, ctypes.byref(par), ctypes.c_void_p(rays_ptr or None), n,
                                                   ctypes.c_void_p(out_ptr or None),
                                                   ctypes.c_void_p(stream_ptr or None)))

    def radiance_stats(self) -> dict:
        """yk_radiance_stats of the last synchronous radiance()."""
        st = RadianceStats()
        _check(self._lib.ykgpu_radiance_get_stats(self._ctx, ctypes.byref(st)))
        return st.as_dict()

    @staticmethod
    def _gather_params(n_samples, max_depth, t_min, rng, linear_scan, count_work) -> GatherParams:
        flags = (records.RADIANCE_LINEAR_SCAN if linear_scan else 0) | (records.RADIANCE_COUNT_WORK if count_work else 0)
        return GatherParams(n_samples, max_depth, rng, flags, t_min, 0)

    def gather(self, points, normals, seeds, n_samples, skip=0, max_depth=50, t_min=records.T_MIN,
               rng=records.RNG_MT19937, linear_scan: bool = False, count_work: bool = False) -> np.ndarray:
        """Diffuse radiance at N points (include/ykgpu.h "gather queries"): points and normals
        float64[N, 3], seeds and skip scalars or uint32[N]; per point n_samples lambertian scatters
        (sample s from Engine(seed + s) with skip words discarded), each followed by ray_color.
        Returns records.GATHER_DTYPE[N]: sum, sumsq, samples, open and flags."""
        return self.gather_points(gather_points(points, normals, seeds, skip), n_samples, max_depth, t_min, rng,
                                  linear_scan, count_work)

    def gather_points(self, points, n_samples, max_depth=50, t_min=records.T_MIN, rng=records.RNG_MT19937,
                      linear_scan: bool = False, count_work: bool = False) -> np.ndarray:
        """gather() on records.GATHER_POINT_DTYPE[N]."""
        pts = np.ascontiguousarray(points, dtype=records.GATHER_POINT_DTYPE).reshape(-1)
        n = pts.size
        out = np.zeros(n, records.GATHER_DTYPE)
        par = self._gather_params(n_samples, max_depth, t_min, rng, linear_scan, count_work)
        _check(self._lib.ykgpu_gather_points(self._ctx, ctypes.byref(par), pts.ctypes.data if n else None, n,
                                             out.ctypes.data if n else None))
        return out

    def gather_device(self, points_ptr: int, n: int, out_ptr: int, n_samples: int, max_depth=50, t_min=records.T_MIN,
                      rng=records.RNG_MT19937, linear_scan: bool = False, count_work: bool = False,
                      stream_ptr: int = 0):
        """Enqueue a gather over device memory (ykgpu_gather_points_async): n yk_gather_point records
        at points_ptr, n yk_gather records written at out_ptr (e.g. [N, 8] float64 CUDA tensors'
        data_ptr()), on the stream (0: the context's).  Does not synchronise."""
        par = self._gather_params(n_samples, max_depth, t_min, rng, linear_scan, count_work)
        _check(self._lib.ykgpu_gather_points_async(self._ctx, ctypes.byref(par), ctypes.c_void_p(points_ptr or None), n,
                                                   ctypes.c_void_p(out_ptr or None),
                                                   ctypes.c_void_p(stream_ptr or None)))

    def gather_stats(self) -> dict:
        """yk_gather_stats of the last synchronous gather()."""
        st = GatherStats()
        _check(self._lib.ykgpu_gather_get_stats(self._ctx, ctypes.byref(st)))
        return st.as_dict()


class Group:
    """Several device contexts in one process (ykgpu_group): rows dealt cyclically over the
    entries, every tile copied into its rows of one host image (include/ykgpu.h)."""

    def __init__(self, devices):
        self._lib = load_library()
        self._g = ctypes.c_void_p()
        self._films = weakref.WeakSet()
        devs = (ctypes.c_int * len(devices))(*devices)
        _check(self._lib.ykgpu_group_create(devs, len(devices), ctypes.byref(self._g)))
        self.devices = list(devices)

    def film(self, params: RenderParams) -> GroupFilm:
        """A group film of the tile `params` names: the single-context film's meaning and bytes."""
        return GroupFilm(self, params)

    def close(self):
        for f in list(self._films):  # films go before their group
            f.close()
        if self._g:
            self._lib.ykgpu_group_destroy(self._g)
            self._g = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def size(self) -> int:
        n = ctypes.c_uint32(0)
        _check(self._lib.ykgpu_group_size(self._g, ctypes.byref(n)))
        return n.value

    def set_scene(self, spheres, camera: Camera):
        arr = spheres if isinstance(spheres, ctypes.Array) else sphere_array(spheres)
        _check(self._lib.ykgpu_group_set_scene(self._g, arr, len(arr), ctypes.byref(camera)))

    def render(self, params: RenderParams) -> np.ndarray:
        out = np.empty((params.row_count, params.tile_width(), 3), np.uint8)
        _check(self._lib.ykgpu_group_render(self._g, ctypes.byref(params), out.ctypes.data))
        return out

    def stats(self, index: int = -1) -> dict:
        st = RenderStats()
        _check(self._lib.ykgpu_group_get_stats(self._g, index, ctypes.byref(st)))
        return st.as_dict()


def render_devices(devices, spheres, camera: Camera, params: RenderParams) -> np.ndarray:
    """ykgpu_render_devices: group, scene, render and release in one call."""
    lib = load_library()
    arr = spheres if isinstance(spheres, ctypes.Array) else sphere_array(spheres)
    devs = (ctypes.c_int * len(devices))(*devices)
    out = np.empty((params.row_count, params.tile_width(), 3), np.uint8)
    _check(lib.ykgpu_render_devices(devs, len(devices), arr, len(arr), ctypes.byref(camera),
                                    ctypes.byref(params), out.ctypes.data))
    return out


__all__ = ["Renderer", "Film", "GroupFilm", "GroupDenoiseStats", "Ray", "Hit", "CastStats", "PathRay", "RadianceParams", "RadianceStats", "camera_sample_rays", "GatherParams", "GatherStats", "gather_points", "gather_sample_rays", "FilmPass", "DenoiseParams", "DenoiseStats", "denoise_defaults", "FeatureParams", "GuidedStats", "guided_defaults", "SampledFeaturesStats", "guided_sampled_defaults", "MattePixel", "MatteStats", "MatteCoverageStats", "scene_hash", "save_film", "load_film", "save_film_counts", "load_film_counts", "Group", "render_devices", "YkError", "build_scene", "write_scene", "read_scene", "SCENE_DIR", "reference_camera", "device_count",
           "make_params", "load_library", "records", "EXPORTS", "LIB_PATH", "CLI_PATH"]
