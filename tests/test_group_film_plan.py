"""The band and exchange plan of a group film's filter (uecraytracing_amd/csrc/yk_group_plan.hpp,
include/ykgpu.h "group films"), through the library's non-ABI helper
yk_group_film_plan (yk_host.cpp; not in include/ykgpu.h).  Pure host code: no GPU.

The render deals tile row t to entry t mod k, where it is row t // k of the entry's sub-tile.  The
plan gives every entry a band of consecutive rows and lists the pitched copies that bring every row
of band +- halo from the entry that rendered it.  Checked exhaustively over rows 1..40, k 1..9 and
halo 0..13 by carrying the copies out on arrays of row numbers."""
import ctypes

import numpy as np
import pytest

import uecraytracing_amd as yk

ROWS, KS, HALOS = range(1, 41), range(1, 10), range(0, 14)


@pytest.fixture(scope="module")
def plan():
    f = yk.load_library().yk_group_film_plan
    f.argtypes = [ctypes.c_uint32] * 3 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    f.restype = ctypes.c_uint32

    def call(rows, k, halo):
        bands = np.zeros((k, 4), np.uint32)
        n = f(rows, k, halo, bands.ctypes.data, None, 0)
        copies = np.zeros((n, 6), np.uint32)
        assert f(rows, k, halo, None, copies.ctypes.data, n) == n
        return bands.astype(np.int64), copies.astype(np.int64)

    return call


def rendered_rows(rows, k, e):
    """The tile rows of entry e's sub-tile, in its order (ykgpu_group_render's dealing)."""
    return list(range(e, rows, k))


def test_the_helper_is_not_part_of_the_abi():
    assert "yk_group_film_plan" not in yk.EXPORTS


@pytest.mark.parametrize("k", KS)
def test_bands_cover_the_tile_once_and_are_clipped(plan, k):
    for rows in ROWS:
        for halo in HALOS:
            bands, _ = plan(rows, k, halo)
            at = 0
            for e, (begin, count, lo, hi) in enumerate(bands):
                assert begin == at, (rows, k, halo, e)  # consecutive, in entry order
                at += count
                # the first rows % k bands are one row taller
                assert count == rows // k + (1 if e < rows % k else 0)
                if count == 0:
                    assert lo == hi
                    continue
                assert lo == max(0, begin - halo) and hi == min(rows, begin + count + halo)
                # a band lies on an entry that holds rows of its own
                assert rendered_rows(rows, k, e)
            assert at == rows  # every tile row owned by exactly one band


@pytest.mark.parametrize("k", KS)
def test_copies_deliver_every_row_once_from_its_renderer(plan, k):
    for rows in ROWS:
        source = [rendered_rows(rows, k, e) for e in range(k)]
        for halo in HALOS:
            bands, copies = plan(rows, k, halo)
            held = [np.full(hi - lo, -1, np.int64) for (_, _, lo, hi) in bands]
            for src, src_row, n, dst, dst_row, pitch in copies:
                assert n > 0 and pitch == k
                assert source[src], "an entry without rows sends nothing"
                assert bands[dst][1] > 0, "an entry without a band receives nothing"
                assert src_row + n <= len(source[src]), (rows, k, halo)  # inside the source's sub-tile
                for i in range(n):
                    at = dst_row + i * pitch
                    assert 0 <= at < len(held[dst]), (rows, k, halo)  # inside the destination's band+halo
                    assert held[dst][at] == -1, "a row delivered twice"
                    held[dst][at] = source[src][src_row + i]
            for e, (_, _, lo, hi) in enumerate(bands):
                # every row of band+halo arrived, at its place, from the entry that rendered it
                assert held[e].tolist() == list(range(lo, hi)), (rows, k, halo, e)
            # one copy per (source, destination) pair at the most
            pairs = [(c[0], c[3]) for c in copies]
            assert len(pairs) == len(set(pairs))


def test_a_few_plans_by_hand(plan):
    # 18 rows over 5 entries at halo 6: bands of 4, 4, 4, 3, 3 rows, shorter than the halo
    bands, copies = plan(18, 5, 6)
    assert bands.tolist() == [[0, 4, 0, 10], [4, 4, 0, 14], [8, 4, 2, 18], [12, 3, 6, 18], [15, 3, 9, 18]]
    # entry 2 holds rows 2..17; entry 0 rendered rows 0, 5, 10, 15: 5, 10, 15 go to rows 3, 8, 13 there
    assert [0, 1, 3, 2, 3, 5] in copies.tolist()
    # a 4-row tile over 5 entries: the last entry renders nothing, owns nothing, and is in no copy
    bands, copies = plan(4, 5, 6)
    assert bands[:, 1].tolist() == [1, 1, 1, 1, 0] and 4 not in copies[:, 0] and 4 not in copies[:, 3]
    assert all(b[2] == 0 and b[3] == 4 for b in bands[:4])  # a halo as tall as the tile
    # one entry: one copy of the whole tile onto itself
    bands, copies = plan(7, 1, 3)
    assert bands.tolist() == [[0, 7, 0, 7]] and copies.tolist() == [[0, 0, 7, 0, 0, 1]]
