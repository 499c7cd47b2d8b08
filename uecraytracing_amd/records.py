"""ctypes mirrors of the plain-C records in include/ykgpu.h (no compute here).

These are the data that cross the C-ABI: the world tuple flattened to ``yk_sphere`` records
(hittable_list.hpp:18-30, sphere.hpp:16-23, material.hpp:37-69), the public members of
``camera<T>`` (camera.hpp:34-37) and the compile-time constants of ``source.cpp:57-66``.
"""
from __future__ import annotations

import ctypes

MATERIAL_LAMBERTIAN = 0
MATERIAL_METAL = 1
MATERIAL_DIELECTRIC = 2

PRECISION_FP64 = 0
PRECISION_FP32 = 1  # render<float> (include/ykgpu.h)
RNG_MT19937 = 0
RNG_XOR128 = 1  # yk::xor128 (random.hpp:18-41), the fast mode (include/ykgpu.h)
SEED_COUNTER = 0
SEED_RANDOM_DEVICE = 1
FLAG_COUNT_WORK = 1
FLAG_LINEAR_SCAN = 2
FLAG_ONE_LANE = 4

YK_OK = 0
ERRORS = {
    1: "YK_ERR_INVALID",
    2: "YK_ERR_DEVICE",
    3: "YK_ERR_NOMEM",
    4: "YK_ERR_UNSUPPORTED",
    5: "YK_ERR_NO_SCENE",
}

T_MIN = 0.001  # raytracer.hpp:27
SEED0_EPOCH0 = 404  # sum of the chars of __TIME__ == "00:00:00" (source.cpp:118-120)

D3 = ctypes.c_double * 3


class Sphere(ctypes.Structure):
    _fields_ = [
        ("center", D3),
        ("radius", ctypes.c_double),
        ("albedo", D3),
        ("fuzz", ctypes.c_double),
        ("ior", ctypes.c_double),
        ("material", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]

    def as_tuple(self):
        return (tuple(self.center), self.radius, tuple(self.albedo), self.fuzz, self.ior,
                self.material)


class Camera(ctypes.Structure):
    _fields_ = [
        ("origin", D3),
        ("lower_left_corner", D3),
        ("horizontal", D3),
        ("vertical", D3),
        ("lens_u", D3),
        ("lens_v", D3),
        ("lens_radius", ctypes.c_double),
    ]

    def as_tuple(self):
        return tuple(tuple(getattr(self, f)) for f, _ in self._fields_[:-1]) + (self.lens_radius,)


class RenderParams(ctypes.Structure):
    _fields_ = [
        ("image_width", ctypes.c_uint32),
        ("image_height", ctypes.c_uint32),
        ("samples_per_pixel", ctypes.c_uint32),
        ("max_depth", ctypes.c_uint32),
        ("seed0", ctypes.c_uint32),
        ("row_begin", ctypes.c_uint32),
        ("row_count", ctypes.c_uint32),
        ("row_stride", ctypes.c_uint32),
        ("precision", ctypes.c_uint32),
        ("rng", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("seed_mode", ctypes.c_uint32),
        ("t_min", ctypes.c_double),
        ("seed_key", ctypes.c_uint64),
        ("row_band_log2", ctypes.c_uint32),  # bands of 2^k rows (include/ykgpu.h)
        ("col_begin", ctypes.c_uint32),  # column set (ABI 10); col_count == 0: every column
        ("col_count", ctypes.c_uint32),
        ("col_stride", ctypes.c_uint32),
        ("col_band_log2", ctypes.c_uint32),
        ("reserved0", ctypes.c_uint32),
    ]

    def tile_width(self) -> int:
        return self.col_count or self.image_width


class RenderStats(ctypes.Structure):
    _fields_ = [
        ("kernel_ms", ctypes.c_double),
        ("resolve_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
        ("warmup_ms", ctypes.c_double),
        ("samples", ctypes.c_uint64),
        ("segments", ctypes.c_uint64),
        ("sphere_tests", ctypes.c_uint64),
        ("sqrt_calls", ctypes.c_uint64),
        ("mt_fallbacks", ctypes.c_uint64),
        ("node_visits", ctypes.c_uint64),
        ("linear_scans", ctypes.c_uint64),
        ("newton_calls", ctypes.c_uint64),
        ("newton_iters", ctypes.c_uint64),
        ("phase_cycles", ctypes.c_uint64 * 8),
        ("timeline", ctypes.c_uint64 * 3),
        ("diag", ctypes.c_uint64 * 4),
        ("seed_key", ctypes.c_uint64),
        ("launches", ctypes.c_uint32),
        ("grid_blocks", ctypes.c_uint32),
        ("render_busy_ms", ctypes.c_double),
        ("work", ctypes.c_uint64 * 8),
        ("device_bytes", ctypes.c_uint64),
        ("call_bytes", ctypes.c_uint64),
        ("sclk_mhz", ctypes.c_double),
        ("launch_spp", ctypes.c_uint32),  # ABI 11
        ("mem_shrinks", ctypes.c_uint32),
    ]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_}
        d["phase_cycles"] = list(self.phase_cycles)
        d["timeline"] = list(self.timeline)
        d["diag"] = list(self.diag)
        d["work"] = list(self.work)
        return d


class FilmStats(ctypes.Structure):
    """yk_film_stats (include/ykgpu.h): the error map's count and maximum."""
    _fields_ = [
        ("pixels", ctypes.c_uint64),
        ("pixels_over", ctypes.c_uint64),  # pixels with e2 > threshold2
        ("max_e2", ctypes.c_double),
        ("samples_done", ctypes.c_uint32),
        ("samples_target", ctypes.c_uint32),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class FilmPass(ctypes.Structure):
    """yk_film_pass (include/ykgpu.h): what one adaptive pass did."""
    _fields_ = [
        ("pixels_selected", ctypes.c_uint64),
        ("samples_added", ctypes.c_uint64),
        ("groups", ctypes.c_uint32),  # distinct (count, take) groups rendered
        ("launches", ctypes.c_uint32),
        ("min_count", ctypes.c_uint32),  # over the tile's pixels, after the pass
        ("max_count", ctypes.c_uint32),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class DenoiseParams(ctypes.Structure):
    """yk_denoise_params (include/ykgpu.h): the non-local-means filter's window, patch and scales."""
    _fields_ = [
        ("radius", ctypes.c_uint32),  # R, 0..10
        ("patch", ctypes.c_uint32),  # F, 0..3
        ("k2", ctypes.c_double),
        ("alpha", ctypes.c_double),
        ("eps", ctypes.c_double),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class DenoiseStats(ctypes.Structure):
    """yk_denoise_stats (include/ykgpu.h): where one ykgpu_film_denoise call spent its time."""
    _fields_ = [
        ("moments_ms", ctypes.c_double),
        ("filter_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class FeatureParams(ctypes.Structure):
    """yk_feature_params (include/ykgpu.h "film features"): the feature pass's grid and the guided
    filter's feature scales."""
    _fields_ = [
        ("grid", ctypes.c_uint32),  # g, 1..4
        ("reserved", ctypes.c_uint32),  # 0
        ("k2", ctypes.c_double),
        ("alpha", ctypes.c_double),
        ("tau_albedo", ctypes.c_double),  # > 0, +inf switches the group off
        ("tau_normal", ctypes.c_double),
        ("tau_depth", ctypes.c_double),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_ if f != "reserved"}


class GroupDenoiseStats(ctypes.Structure):
    """yk_group_denoise_stats (include/ykgpu.h "group films"): where one group film filter call spent
    its time, each device time the largest entry's."""
    _fields_ = [
        ("features_ms", ctypes.c_double),  # 0 for the colour-only filter and when the pass was cached
        ("moments_ms", ctypes.c_double),
        ("exchange_ms", ctypes.c_double),
        ("filter_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class GuidedStats(ctypes.Structure):
    """yk_guided_stats (include/ykgpu.h): where one ykgpu_film_denoise_guided call spent its time."""
    _fields_ = [
        ("features_ms", ctypes.c_double),  # 0 when the cached pass was reused
        ("moments_ms", ctypes.c_double),
        ("filter_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class SampledFeaturesStats(ctypes.Structure):
    """yk_sampled_features_stats (include/ykgpu.h "sampled film features"): the pass that made a film's
    sampled feature planes."""
    _fields_ = [
        ("ms", ctypes.c_double),  # 0 when the cached pass was reused
        ("samples", ctypes.c_uint64),  # pixels * n
        ("hits", ctypes.c_uint64),
        ("redo_pixels", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_ if f != "reserved"}


MATTE_SKY = 0xFFFFFFFF  # YK_MATTE_SKY: the sky among a matte's ids, and the id of an unused slot
MATTE_SLOTS = 8


class MattePixel(ctypes.Structure):
    """yk_matte_pixel (include/ykgpu.h "film mattes"): the id-coverage table of one pixel."""
    _fields_ = [
        ("id", ctypes.c_uint32 * 8),  # by count descending, equal counts by id ascending; unused: MATTE_SKY
        ("count", ctypes.c_uint32 * 8),
        ("n", ctypes.c_uint32),  # sum(count) + miss + other
        ("miss", ctypes.c_uint32),
        ("other", ctypes.c_uint32),  # hits that found the 8 slots taken by other ids
        ("used", ctypes.c_uint32),
    ]


class MatteStats(ctypes.Structure):
    """yk_matte_stats (include/ykgpu.h "film mattes"): the pass that made a film's matte table."""
    _fields_ = [
        ("ms", ctypes.c_double),  # 0 when the cached table was reused
        ("samples", ctypes.c_uint64),  # the sum of n over the pixels
        ("hits", ctypes.c_uint64),
        ("other_samples", ctypes.c_uint64),
        ("overflow_pixels", ctypes.c_uint32),  # pixels with other > 0
        ("redo_pixels", ctypes.c_uint32),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class MatteCoverageStats(ctypes.Structure):
    """yk_matte_coverage_stats (include/ykgpu.h "film mattes"): one coverage call."""
    _fields_ = [
        ("ms", ctypes.c_double),
        ("pixels_selected", ctypes.c_uint64),  # pixels with sel > 0
        ("pixels_uncertain", ctypes.c_uint64),  # pixels with other > 0
        ("samples_selected", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


HIT_HIT = 1  # yk_hit.flags (include/ykgpu.h "ray queries")
HIT_FRONT_FACE = 2
HIT_OUT_OF_DOMAIN = 4
CAST_ANY_HIT = 1  # ykgpu_cast_rays' flags
CAST_LINEAR_SCAN = 2
CAST_COUNT_WORK = 4
NO_HIT_ID = 0xFFFFFFFF


class Ray(ctypes.Structure):
    """yk_ray (include/ykgpu.h "ray queries"): origin, direction and the limits of one ray."""
    _fields_ = [
        ("origin", D3),
        ("direction", D3),
        ("t_min", ctypes.c_double),
        ("t_max", ctypes.c_double),  # may be +inf
    ]


class Hit(ctypes.Structure):
    """yk_hit (include/ykgpu.h): the hit_record of one ray, the sphere's tuple index and HIT_* flags."""
    _fields_ = [
        ("p", D3),
        ("normal", D3),
        ("t", ctypes.c_double),
        ("id", ctypes.c_uint32),  # NO_HIT_ID when none
        ("flags", ctypes.c_uint32),
    ]


class CastStats(ctypes.Structure):
    """yk_cast_stats (include/ykgpu.h): what the last synchronous ykgpu_cast_rays did."""
    _fields_ = [
        ("kernel_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
        ("rays", ctypes.c_uint64),
        ("hits", ctypes.c_uint64),
        ("out_of_domain", ctypes.c_uint64),
        ("scan_rays", ctypes.c_uint64),  # rays served by the ordered scan
        ("node_visits", ctypes.c_uint64),  # CAST_COUNT_WORK only, else 0
        ("sphere_tests", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


def _np_dtype(names, formats, itemsize):
    import numpy as np
    return np.dtype({"names": names, "formats": formats, "itemsize": itemsize})


# numpy views of yk_ray and yk_hit: arrays of these dtypes are the C records, byte for byte
RAY_DTYPE = _np_dtype(["origin", "direction", "t_min", "t_max"], [("<f8", 3), ("<f8", 3), "<f8", "<f8"], 64)
HIT_DTYPE = _np_dtype(["p", "normal", "t", "id", "flags"], [("<f8", 3), ("<f8", 3), "<f8", "<u4", "<u4"], 64)
# ... and of yk_matte_pixel
MATTE_DTYPE = _np_dtype(["id", "count", "n", "miss", "other", "used"], [("<u4", 8), ("<u4", 8), "<u4", "<u4", "<u4", "<u4"], 80)

RAD_SKY = 1  # yk_radiance.flags (include/ykgpu.h "radiance queries"): how the path ended
RAD_ABSORBED = 2
RAD_DEPTH = 4
RAD_OUT_OF_DOMAIN = 8
RAD_MT_FALLBACK = 16  # beside one of the above: the path drew more than 227 mt19937 words
RADIANCE_LINEAR_SCAN = 1  # yk_radiance_params.flags
RADIANCE_COUNT_WORK = 2


class PathRay(ctypes.Structure):
    """yk_path_ray (include/ykgpu.h "radiance queries"): a ray and its path's engine (seed, skip)."""
    _fields_ = [
        ("origin", D3),
        ("direction", D3),
        ("seed", ctypes.c_uint32),
        ("skip", ctypes.c_uint32),  # engine words discarded before ray_color's first draw
        ("reserved", ctypes.c_uint64),
    ]


class RadianceParams(ctypes.Structure):
    """yk_radiance_params (include/ykgpu.h): ray_color's depth, the engine, t_min and RADIANCE_* flags."""
    _fields_ = [
        ("max_depth", ctypes.c_uint32),  # 1..65535
        ("rng", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("t_min", ctypes.c_double),
        ("reserved1", ctypes.c_uint64),
    ]


class RadianceStats(ctypes.Structure):
    """yk_radiance_stats (include/ykgpu.h): what the last synchronous ykgpu_radiance_rays did."""
    _fields_ = [
        ("kernel_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
        ("starts_ms", ctypes.c_double),  # the part of kernel_ms in the starts kernel
        ("rays", ctypes.c_uint64),
        ("segments", ctypes.c_uint64),  # RADIANCE_COUNT_WORK only, else 0
        ("words", ctypes.c_uint64),
        ("out_of_domain", ctypes.c_uint32),
        ("mt_fallbacks", ctypes.c_uint32),
        ("scan_segments", ctypes.c_uint32),  # RADIANCE_COUNT_WORK only
        ("lanes", ctypes.c_uint32),  # resident lanes of the path kernel's grid
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


assert ctypes.sizeof(PathRay) == 64 and ctypes.sizeof(RadianceParams) == 32 and ctypes.sizeof(RadianceStats) == 64
assert ctypes.sizeof(Ray) == 64 and ctypes.sizeof(Hit) == 64 and ctypes.sizeof(CastStats) == 64
# ... and of yk_path_ray and yk_radiance
PATH_RAY_DTYPE = _np_dtype(["origin", "direction", "seed", "skip", "reserved"],
                           [("<f8", 3), ("<f8", 3), "<u4", "<u4", "<u8"], 64)
RADIANCE_DTYPE = _np_dtype(["colour", "t_first", "id_first", "id_last", "words", "segments", "flags", "reserved"],
                           [("<f8", 3), "<f8", "<u4", "<u4", "<u4", "<u4", "<u4", ("<u4", 3)], 64)
assert RAY_DTYPE.itemsize == 64 and HIT_DTYPE.itemsize == 64
assert PATH_RAY_DTYPE.itemsize == 64 and RADIANCE_DTYPE.itemsize == 64
assert RADIANCE_DTYPE.fields["flags"][1] == 48 and PATH_RAY_DTYPE.fields["seed"][1] == 48
GATHER_MAX_SKIP = 221  # yk_gather_point.skip (include/ykgpu.h "gather queries"): past it, out of domain
GATHER_MAX_SAMPLES = 65536


class GatherPoint(ctypes.Structure):
    """yk_gather_point (include/ykgpu.h "gather queries"): a point, its normal and its samples' engines."""
    _fields_ = [
        ("p", D3),
        ("n", D3),  # used as given, never normalised
        ("seed", ctypes.c_uint32),  # sample s draws from Engine(seed + s)
        ("skip", ctypes.c_uint32),  # engine words discarded before the scatter's draws; <= GATHER_MAX_SKIP
        ("reserved", ctypes.c_uint64),
    ]


class Gather(ctypes.Structure):
    """yk_gather (include/ykgpu.h): the fold of a point's samples."""
    _fields_ = [
        ("sum", D3),
        ("sumsq", D3),
        ("samples", ctypes.c_uint32),
        ("open", ctypes.c_uint32),  # samples whose gather ray hit nothing
        ("flags", ctypes.c_uint32),  # RAD_OUT_OF_DOMAIN | RAD_MT_FALLBACK of any sample
        ("reserved", ctypes.c_uint32),
    ]


class GatherParams(ctypes.Structure):
    """yk_gather_params (include/ykgpu.h): samples per point, ray_color's depth, the engine, RADIANCE_* flags, t_min."""
    _fields_ = [
        ("n_samples", ctypes.c_uint32),  # 1..GATHER_MAX_SAMPLES
        ("max_depth", ctypes.c_uint32),  # 1..65535
        ("rng", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("t_min", ctypes.c_double),
        ("reserved", ctypes.c_uint64),
    ]


class GatherStats(ctypes.Structure):
    """yk_gather_stats (include/ykgpu.h): what the last synchronous ykgpu_gather_points did."""
    _fields_ = [
        ("kernel_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
        ("starts_ms", ctypes.c_double),  # the parts of kernel_ms in the starts and the fold kernel
        ("fold_ms", ctypes.c_double),
        ("points", ctypes.c_uint64),
        ("rays", ctypes.c_uint64),
        ("open", ctypes.c_uint64),
        ("out_of_domain", ctypes.c_uint32),  # points, not rays
        ("mt_fallbacks", ctypes.c_uint32),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


# numpy views of yk_gather_point and yk_gather
GATHER_POINT_DTYPE = _np_dtype(["p", "n", "seed", "skip", "reserved"], [("<f8", 3), ("<f8", 3), "<u4", "<u4", "<u8"], 64)
GATHER_DTYPE = _np_dtype(["sum", "sumsq", "samples", "open", "flags", "reserved"],
                         [("<f8", 3), ("<f8", 3), "<u4", "<u4", "<u4", "<u4"], 64)
assert ctypes.sizeof(GatherPoint) == 64 and ctypes.sizeof(Gather) == 64
assert ctypes.sizeof(GatherParams) == 32 and ctypes.sizeof(GatherStats) == 64
assert GATHER_POINT_DTYPE.itemsize == 64 and GATHER_DTYPE.itemsize == 64
assert GATHER_POINT_DTYPE.fields["seed"][1] == 48 and GATHER_DTYPE.fields["samples"][1] == 48
assert ctypes.sizeof(Sphere) == 80
assert ctypes.sizeof(FeatureParams) == 48
assert ctypes.sizeof(GuidedStats) == 32
assert ctypes.sizeof(DenoiseParams) == 32
assert ctypes.sizeof(DenoiseStats) == 24
assert ctypes.sizeof(FilmPass) == 32
assert ctypes.sizeof(FilmStats) == 32
assert ctypes.sizeof(Camera) == 19 * 8
assert ctypes.sizeof(RenderParams) == 88
assert ctypes.sizeof(RenderStats) == 344


def image_height_for(width: int) -> int:
    """uint32(W / (16.0/9.0)), source.cpp:59-62."""
    return int(width / (16.0 / 9.0))


def make_params(width, height=None, spp=8, max_depth=50, seed0=SEED0_EPOCH0, rows=None,
                flags=0, t_min=T_MIN, precision=PRECISION_FP64, seed_mode=SEED_COUNTER,
                seed_key=0, rng=RNG_MT19937, cols=None) -> RenderParams:
    """rows = (row_begin, row_count, row_stride[, row_band_log2]); default: the whole image.
    cols = (col_begin, col_count, col_stride[, col_band_log2]); default: every column."""
    if height is None:
        height = image_height_for(width)
    rb, rc, rs, band = (tuple(rows) + (0,))[:4] if rows is not None else (0, height, 1, 0)
    cb, cc, cs, cband = (tuple(cols) + (0,))[:4] if cols is not None else (0, 0, 0, 0)
    return RenderParams(width, height, spp, max_depth, seed0 & 0xFFFFFFFF, rb, rc, rs,
                        precision, rng, flags, seed_mode, t_min, seed_key, band, cb, cc, cs, cband, 0)


def sphere_array(spheres) -> ctypes.Array:
    arr = (Sphere * len(spheres))()
    for i, s in enumerate(spheres):
        arr[i] = s
    return arr


def lambertian(center, radius, albedo) -> Sphere:
    return Sphere(D3(*center), radius, D3(*albedo), 0.0, 0.0, MATERIAL_LAMBERTIAN, 0)


def metal(center, radius, albedo, fuzz=0.0) -> Sphere:
    return Sphere(D3(*center), radius, D3(*albedo), fuzz, 0.0, MATERIAL_METAL, 0)


def dielectric(center, radius, ior) -> Sphere:
    return Sphere(D3(*center), radius, D3(1.0, 1.0, 1.0), 0.0, ior, MATERIAL_DIELECTRIC, 0)
