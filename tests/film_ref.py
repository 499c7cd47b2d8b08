"""The yardstick of the film tests (TEST INFRASTRUCTURE ONLY): the oracle's per-sample colours
(oracle_lib.sample, yko_sample) folded in numpy, in sample order — not the code under test.

  sums   s = ((0 + c_0) + c_1) + ...        the reference's left fold (source.cpp:137-167)
  sumsq  q = q + (c * c)                    product rounded, then the sum (numpy never fuses)
  e2     max(0, v_r, v_g, v_b),  v = (q - (s*s)/n) / (n*(n-1))
  image  to_color3b(s, n): /n, math::sqrt, clamp [0, .999], *256, truncate (source.cpp:73-83)

Every array operation here is one IEEE double operation per element, so the GPU film must equal
these bytes exactly.  The colours of a (scene, params) pair are computed once and shared."""
import ctypes

import numpy as np

import oracle_lib

_cache = {}


def tile_rows(p):
    L = p.row_band_log2
    return [p.row_begin + ((i >> L) * p.row_stride << L) + (i & ((1 << L) - 1)) for i in range(p.row_count)]


def tile_cols(p):
    if not p.col_count:
        return list(range(p.image_width))
    L = p.col_band_log2
    return [p.col_begin + ((j >> L) * p.col_stride << L) + (j & ((1 << L) - 1)) for j in range(p.col_count)]


def colours(spheres, camera, p) -> np.ndarray:
    """float64[row_count, tile width, spp, 3]: the oracle's colour of every sample of the tile
    (read-only, cached)."""
    arr = spheres if isinstance(spheres, ctypes.Array) else oracle_lib.sphere_array(spheres)
    key = (bytes(arr), bytes(camera), bytes(p))
    if key not in _cache:
        ys, xs = tile_rows(p), tile_cols(p)
        out = np.empty((len(ys), len(xs), p.samples_per_pixel, 3), np.float64)
        for i, y in enumerate(ys):
            for j, x in enumerate(xs):
                for s in range(p.samples_per_pixel):
                    out[i, j, s] = oracle_lib.sample(arr, camera, p, y, x, s)[0]
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def prefixes(cols: np.ndarray):
    """(S, Q): S[k], Q[k] the sums and second moments after the first k samples, k = 0..spp."""
    s = np.zeros(cols.shape[:2] + (3,), np.float64)
    q = np.zeros_like(s)
    S, Q = [s], [q]
    for k in range(cols.shape[2]):
        c = cols[:, :, k, :]
        s = s + c
        q = q + (c * c)
        S.append(s)
        Q.append(q)
    return S, Q


def to_color3b(sums: np.ndarray, n: int) -> np.ndarray:
    v = oracle_lib.newton_sqrt_array(sums / float(n))
    v = np.where(v < 0.0, 0.0, np.where(0.999 < v, 0.999, v))
    return (v * 256).astype(np.uint32).astype(np.uint8)


def e2_map(sums: np.ndarray, sumsq: np.ndarray, n: int) -> np.ndarray:
    n = float(n)
    v = (sumsq - (sums * sums) / n) / (n * (n - 1.0))
    e2 = np.zeros(sums.shape[:2], np.float64)
    for c in range(3):
        e2 = np.where(v[:, :, c] > e2, v[:, :, c], e2)
    return e2
