"""The seed table's index and key (uecraytracing_amd/csrc/yk_seed_table.hpp), on the
CPU: every (sample, tile pixel) of a tile maps to a distinct word below the table's size, and the
seed that word stands for is the counter seed of that sample of that image pixel,
seed0 + (y*W + x)*spp + s in uint32 arithmetic (ykd::sample_seed), for odd tile shapes, banded rows
and column bands.  tests/test_gpu_seed_table.py runs the kernels that use the index."""
import os
import subprocess

import numpy as np
import pytest

from uecraytracing_amd import tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("seed_table") / "seed_table_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "seed_table_driver.cpp")], check=True)
    return exe


def image_coords(count, begin, stride, band_log2):
    """image row (column) of each tile row (column): bands of 2^band_log2, every stride-th band"""
    B = 1 << band_log2
    return [begin + (t // B) * stride * B + t % B for t in range(count)]


# (seed0, W, H, spp, rows, cols): rows / cols as the C-ABI takes them (begin, count, stride, band_log2);
# cols None: every column
CASES = {
    "whole-odd": (404, 37, 23, 5, (0, 23, 1, 0), None),
    "one-pixel": (7, 1, 1, 1, (0, 1, 1, 0), None),
    "rows-1-of-2": (404, 72, 40, 6, tiles.tile_rows(1, 2, 40), None),
    "rows-2-of-3-odd": (404, 37, 23, 3, tiles.tile_rows(2, 3, 23), None),
    "row-bands-of-2": (404, 19, 23, 4, tiles.tile_rows(1, 3, 23, 1), None),  # (a partial last band)
    "row-bands-of-8": (404, 19, 43, 2, tiles.tile_rows(0, 2, 43, 3), None),
    "col-bands-of-8": (404, 72, 11, 6, (0, 11, 1, 0), tiles.tile_cols(0, 2, 72)),
    "col-bands-partial": (404, 45, 9, 3, (0, 9, 1, 0), tiles.tile_cols(1, 3, 45)),  # (45 = 5 bands + 5 columns)
    "rows-and-cols": (404, 45, 23, 3, tiles.tile_rows(1, 2, 23), tiles.tile_cols(0, 2, 45, 2)),
    "seed-wraps": (4294967000, 48, 27, 4, (0, 27, 1, 0), None),
    "single-columns": (12345, 21, 5, 2, (0, 5, 1, 0), tiles.tile_cols(2, 4, 21, 0)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_index_and_seed(driver, name):
    seed0, W, H, spp, rows, cols = CASES[name]
    c = cols or (0, 0, 0, 0)
    out = subprocess.run([driver, *(str(v) for v in (seed0, W, spp, *rows, *c))], check=True, capture_output=True,
                         text=True).stdout.split()
    ys = image_coords(rows[1], rows[0], rows[2], rows[3])
    xs = image_coords(cols[1], cols[0], cols[2], cols[3]) if cols else list(range(W))
    assert max(ys) < H and max(xs) < W and len(set(ys)) == len(ys) and len(set(xs)) == len(xs)
    T = len(ys) * len(xs)
    # (the driver has checked that the T * spp indices are distinct and below the size)
    assert int(out[0]) == T and int(out[1]) == T * spp and len(out) == 2 + T * spp
    got = np.array(out[2:], dtype=np.uint64)
    y, x = np.meshgrid(np.array(ys, np.uint64), np.array(xs, np.uint64), indexing="ij")  # tile pixel q = t * Wt + j
    pix = (y * W + x).reshape(-1)
    want = (seed0 + pix[None, :] * spp + np.arange(spp, dtype=np.uint64)[:, None]) % (1 << 32)  # tab[s * T + q]
    np.testing.assert_array_equal(got, want.reshape(-1))
    if name == "seed-wraps":
        assert want.min() < 1000 and want.max() > 4294967000, "the case's seeds cross 2^32"


def test_tile_helpers_agree_with_the_package():
    """image_coords above is tiles.tile_image_rows' dealing, so the cases are the tiles the N-GPU split makes."""
    for world, n, band in ((2, 40, 0), (3, 23, 1), (2, 43, 3), (3, 45, 3)):
        for rank in range(world):
            begin, count, stride, b = tiles.tile_rows(rank, world, n, band)
            assert image_coords(count, begin, stride, b) == tiles.tile_image_rows(rank, world, n, band)
