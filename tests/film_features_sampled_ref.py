"""The yardstick of the sampled-feature tests (TEST INFRASTRUCTURE ONLY): include/ykgpu.h "sampled
film features" / DESIGN.md §6.8 restated in numpy — not the code under test.

Per pixel (x, y) of the tile and s = 0 .. n-1 in order:
  (o, d) = radiance_ref.camera_start(camera, p, y, x, s)     the render's own start ray of sample s
  a ray outside cast_ref.in_domain is a miss; otherwise the hit is cast_ref.scan's (t_min = p.t_min,
  t_max = +inf, ties to the later index)
  f = (albedo | 1,1,1 for a dielectric, face-forward normal, t), a miss (1,1,1, 0,0,0, 0)
  s = s + f, q = q + (f*f);  G = n
  F = s / G,  U = max(0, (q - (s*s)/G) / (G*(G - 1)))  (n = 1: U = 0)
Every array statement is one IEEE double operation per element, so the GPU must equal these bytes
exactly.  The guided filter on these planes is film_features_ref.guided_nlm, unchanged."""
import numpy as np

import cast_ref
import film_denoise_ref as fdr
import film_features_ref as ffr
import film_ref
import oracle_lib
import radiance_ref

INF = float("inf")
MATERIAL_DIELECTRIC = 2
MAX_SAMPLES = 256

_cache = {}


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def first_hits(spheres, camera, p, n):
    """(o, d float64[rows, wt, n, 3], hit int64[rows, wt, n], t float64[rows, wt, n]): the start ray of
    every pixel's samples 0..n-1 and its closest hit (hit -1: a miss, t then +inf)."""
    spheres = list(spheres)
    rows, cols = film_ref.tile_rows(p), film_ref.tile_cols(p)
    o = np.empty((len(rows), len(cols), n, 3), np.float64)
    d = np.empty_like(o)
    for i, y in enumerate(rows):
        for j, x in enumerate(cols):
            for s in range(n):
                o[i, j, s], d[i, j, s], _, _ = radiance_ref.camera_start(camera, p, int(y), int(x), s)
    of, df = o.reshape(-1, 3).copy(), d.reshape(-1, 3).copy()
    t_min = np.full(len(of), np.float64(p.t_min))
    t_max = np.full(len(of), INF)
    dom = cast_ref.in_domain(of, df, t_min, t_max, cast_ref.extent(spheres))
    # rays outside the domain do no arithmetic: a harmless ray stands in for them
    of[~dom], df[~dom] = 0.0, (0.0, 0.0, -1.0)
    t, hit = cast_ref.scan(spheres, of, df, t_min, t_max)
    hit = np.where(dom, hit, -1)
    t = np.where(hit >= 0, t, INF)
    return o, d, hit.reshape(o.shape[:3]), t.reshape(o.shape[:3])


def channels(spheres, o, d, hit, t):
    """f float64[..., 7] of rays o, d [..., 3] with their hits."""
    spheres = list(spheres)
    cen = np.array([tuple(s.center) for s in spheres], np.float64).reshape(-1, 3)
    rad = np.array([s.radius for s in spheres], np.float64)
    alb = np.array([(1.0, 1.0, 1.0) if s.material == MATERIAL_DIELECTRIC else tuple(s.albedo) for s in spheres],
                   np.float64).reshape(-1, 3)
    found = hit >= 0
    k = np.where(found, hit, 0)
    tt = np.where(found, t, 1.0)
    f = np.zeros(hit.shape + (7,), np.float64)
    f[..., 0:3] = 1.0
    if not len(spheres):
        return f
    with np.errstate(invalid="ignore", over="ignore"):
        pt = [o[..., c] + d[..., c] * tt for c in range(3)]
        outward = [(pt[c] - cen[k, c]) / rad[k] for c in range(3)]
        front = _dot([d[..., c] for c in range(3)], outward) < 0
    for c in range(3):
        f[..., c] = np.where(found, alb[k, c], 1.0)
        f[..., 3 + c] = np.where(found, np.where(front, outward[c], -outward[c]), 0.0)
    f[..., 6] = np.where(found, t, 0.0)
    return f


def features(spheres, camera, p, n):
    """(F, U float64[row_count, tile width, 7], stats dict): the sampled feature means, the variances
    of the means, and the pass's samples and hits (read-only, cached)."""
    arr = spheres if not isinstance(spheres, list) else oracle_lib.sphere_array(spheres)
    key = (bytes(arr), bytes(camera), bytes(p), int(n))
    if key in _cache:
        return _cache[key]
    n = int(n)
    assert 1 <= n <= min(MAX_SAMPLES, p.samples_per_pixel)
    o, d, hit, t = first_hits(list(arr), camera, p, n)
    f = channels(list(arr), o, d, hit, t)
    s = np.zeros(hit.shape[:2] + (7,), np.float64)
    q = np.zeros_like(s)
    for k in range(n):
        s = s + f[:, :, k]
        q = q + (f[:, :, k] * f[:, :, k])
    G = np.float64(n)
    F = s / G
    if n >= 2:
        U = (q - (s * s) / G) / (G * (G - 1.0))
        U = np.where(U > 0.0, U, 0.0)
    else:
        U = np.zeros_like(F)
    F, U = np.ascontiguousarray(F), np.ascontiguousarray(U)
    for a in (F, U):
        a.setflags(write=False)
    out = (F, U, dict(samples=int(hit.size), hits=int((hit >= 0).sum())))
    _cache[key] = out
    return out


def denoise_guided(sums, sumsq, counts, spheres, camera, p, n, colour=None, feat=None):
    """film_features_ref.denoise_guided with the sampled planes of the first n samples as guides."""
    kw, _ = ffr.split(colour, feat)
    m, v = fdr.moments(sums, sumsq, counts)
    F, U, _ = features(spheres, camera, p, n)
    return ffr.guided_nlm(m, v, F, U, **kw)
