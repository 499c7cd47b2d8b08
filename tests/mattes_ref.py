"""The yardstick of the film-matte tests (TEST INFRASTRUCTURE ONLY): include/ykgpu.h "film mattes" /
DESIGN.md §6.10 restated in Python and numpy — not the code under test.

Per pixel (x, y) of the tile, n_p its sample count, for s = 0 .. n_p-1 in order:
  the sample's first hit is film_features_sampled_ref.first_hits' (the render's own start ray, the
  ordered scan with t_min = p.t_min and t_max = +inf, a ray outside the domain a miss)
  a miss: miss += 1; a hit on a sphere that holds one of the 8 slots: that slot's count += 1; a hit
  on another sphere while fewer than 8 slots are in use: a new slot (k, 1); otherwise other += 1
  the record: the slots by count descending, equal counts by id ascending, unused slots (SKY, 0)
Coverage of a set of ids: sel = the selected slots' counts (+ miss when SKY is among the ids),
cov = sel / n in double (0.0 where n = 0), grey = trunc(clamp(cov, 0, 0.999) * 256).
Everything but that one division is integer arithmetic, so the GPU must equal these bytes."""
import numpy as np

import film_features_sampled_ref as fsr
import oracle_lib
from uecraytracing_amd.records import MATTE_DTYPE, MATTE_SKY, MATTE_SLOTS

SLOTS, SKY = MATTE_SLOTS, MATTE_SKY
assert MATTE_DTYPE.itemsize == 80 and SLOTS == 8

_hits = {}
_tables = {}


def fold_ids(ids):
    """The record of one pixel from its samples' first-hit ids in sample order (-1: a miss), as a
    dict: id and count (lists of 8), n, miss, other, used."""
    slots, miss, other = [], 0, 0  # [id, count] in the order the ids came
    for k in ids:
        k = int(k)
        if k < 0:
            miss += 1
            continue
        held = [s for s in slots if s[0] == k]
        if held:
            held[0][1] += 1
        elif len(slots) < SLOTS:
            slots.append([k, 1])
        else:
            other += 1
    order = sorted(slots, key=lambda s: (-s[1], s[0]))
    pad = SLOTS - len(order)
    return dict(id=[s[0] for s in order] + [SKY] * pad, count=[s[1] for s in order] + [0] * pad, n=len(ids), miss=miss,
                other=other, used=len(order))


def first_hit_ids(spheres, camera, p, n):
    """int64[row_count, tile width, n]: the first-hit id of every pixel's samples 0..n-1 (read-only, cached)."""
    arr = spheres if not isinstance(spheres, list) else oracle_lib.sphere_array(spheres)
    key = (bytes(arr), bytes(camera), bytes(p), int(n))
    if key not in _hits:
        hit = fsr.first_hits(list(arr), camera, p, int(n))[2]
        hit.setflags(write=False)
        _hits[key] = hit
    return _hits[key]


def table(spheres, camera, p, n):
    """(records MATTE_DTYPE[row_count, tile width], stats dict): the table of the first n samples, n an
    int, or of each pixel's own count, n a uint32[row_count, tile width] array (read-only, cached)."""
    arr = spheres if not isinstance(spheres, list) else oracle_lib.sphere_array(spheres)
    counts = None if np.isscalar(n) else np.ascontiguousarray(n, dtype=np.uint32)
    key = (bytes(arr), bytes(camera), bytes(p), int(n) if counts is None else counts.tobytes())
    if key in _tables:
        return _tables[key]
    rows, wt = p.row_count, p.tile_width()
    if counts is None:
        counts = np.full((rows, wt), int(n), np.uint32)
    assert counts.shape == (rows, wt) and int(counts.max(initial=0)) <= p.samples_per_pixel
    top = int(counts.max(initial=0))
    hit = first_hit_ids(arr, camera, p, top) if top else np.zeros((rows, wt, 0), np.int64)
    out = np.zeros((rows, wt), MATTE_DTYPE)
    hits = 0
    for i in range(rows):
        for j in range(wt):
            ids = hit[i, j, :int(counts[i, j])]
            rec = fold_ids(ids)
            for f in MATTE_DTYPE.names:
                out[i, j][f] = rec[f]
            hits += int((ids >= 0).sum())
    out.setflags(write=False)
    stats = dict(samples=int(counts.sum(dtype=np.uint64)), hits=hits, other_samples=int(out["other"].sum(dtype=np.uint64)),
                 overflow_pixels=int((out["other"] > 0).sum()))
    _tables[key] = (out, stats)
    return _tables[key]


def coverage(tab, ids):
    """(cov float64, grey uint8, stats dict) of a table for a set of ids (duplicates count once)."""
    want = sorted({int(k) for k in ids})
    assert want
    sel = np.zeros(tab.shape, np.uint64)
    for k in want:
        if k == SKY:
            sel += tab["miss"]
        else:
            sel += np.where((tab["id"] == k) & (tab["count"] > 0), tab["count"], 0).sum(axis=-1, dtype=np.uint64)
    n = tab["n"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        cov = np.where(tab["n"] == 0, 0.0, sel.astype(np.float64) / n)
    grey = np.trunc(np.clip(cov, 0.0, 0.999) * 256.0).astype(np.uint8)
    stats = dict(pixels_selected=int((sel > 0).sum()), pixels_uncertain=int((tab["other"] > 0).sum()),
                 samples_selected=int(sel.sum(dtype=np.uint64)))
    return np.ascontiguousarray(cov), np.ascontiguousarray(grey), stats
