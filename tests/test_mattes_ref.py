"""The film mattes' host side (no device): the restatement (mattes_ref) pinned on its own — the table
rule on hand-written id sequences, the invariant, its hits against the sampled feature yardstick and
the first segment radiance_ref.ray_color records — and the populations the GPU tests rely on: pixels
with more than 8 distinct ids, with exactly 8 and with fewer in many(700), none above 4 in final48.
The new records and entry points are checked against the header.  The GPU tests
(test_gpu_film_mattes.py) compare the library with mattes_ref byte for byte.
"""
import ctypes
import os

import numpy as np
import pytest

import cast_ref
import edge_inputs
import film_features_ref as ffr
import film_features_sampled_ref as fsr
import mattes_ref as mr
import radiance_ref as rr
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd import records
from uecraytracing_amd.records import make_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = refscenes.reference_camera()
SKY = records.MATTE_SKY


def test_fold_ids_on_hand_written_sequences():
    # counts descending, the tie of 5 and 9 (two each) by id ascending
    r = mr.fold_ids([9, 5, -1, 9, 7, 5, 7, 7])
    assert r == dict(id=[7, 5, 9] + [SKY] * 5, count=[3, 2, 2] + [0] * 5, n=8, miss=1, other=0, used=3)
    # a ninth distinct id goes to `other`, whatever comes after it; the first 8 keep counting
    seq = [10, 11, 12, 13, 14, 15, 16, 17, 18, 18, 10, 19, 17, -1]
    r = mr.fold_ids(seq)
    assert r["id"] == [10, 17, 11, 12, 13, 14, 15, 16] and r["count"] == [2, 2, 1, 1, 1, 1, 1, 1]
    assert (r["n"], r["miss"], r["other"], r["used"]) == (14, 1, 3, 8)
    # the rule depends on the order: the same ids, the ninth first
    r2 = mr.fold_ids([18] + seq)
    assert 18 in r2["id"] and 17 not in r2["id"] and r2["other"] == 3 and r2["count"][0] == 3
    # every sample a miss, and no sample at all
    assert mr.fold_ids([-1] * 5) == dict(id=[SKY] * 8, count=[0] * 8, n=5, miss=5, other=0, used=0)
    assert mr.fold_ids([]) == dict(id=[SKY] * 8, count=[0] * 8, n=0, miss=0, other=0, used=0)
    # exactly 8 distinct ids: no overflow
    r = mr.fold_ids(list(range(8, 0, -1)))
    assert r["id"] == list(range(1, 9)) and r["other"] == 0 and r["used"] == 8


def check_invariant(tab):
    assert (tab["count"].sum(axis=-1, dtype=np.uint64) + tab["miss"] + tab["other"] == tab["n"]).all()
    assert ((tab["count"] > 0).sum(axis=-1) == tab["used"]).all()
    assert ((tab["id"] == SKY) == (tab["count"] == 0)).all()
    c = tab["count"].astype(np.int64)
    assert (c[..., :-1] >= c[..., 1:]).all()  # by count descending ...
    tie = (c[..., :-1] == c[..., 1:]) & (c[..., 1:] > 0)
    assert (tab["id"][..., :-1][tie] < tab["id"][..., 1:][tie]).all()  # ... equal counts by id ascending


@pytest.fixture(scope="module")
def many700():
    scene = ffr.many(700)
    p = make_params(16, 9, 32, 50, 404)
    return scene, p, mr.table(scene, CAM, p, 32)


def test_many700_has_every_population(many700):
    scene, p, (tab, st) = many700
    check_invariant(tab)
    distinct = np.array([[len(set(int(k) for k in row if k >= 0)) for row in line] for line in mr.first_hit_ids(scene, CAM, p, 32)])
    over, exact, fewer = int((distinct > 8).sum()), int((distinct == 8).sum()), int((distinct < 8).sum())
    assert (over, exact, fewer) == (13, 7, 124)
    assert int((tab["miss"] > 0).sum()) == 70
    assert st["overflow_pixels"] == over == int((tab["other"] > 0).sum()) and st["other_samples"] >= over
    assert ((tab["used"] == 8) == (distinct >= 8)).all()
    assert st["samples"] == 16 * 9 * 32 and st["hits"] == fsr.features(scene, CAM, p, 32)[2]["hits"]
    assert st["hits"] == int(tab["count"].sum(dtype=np.uint64)) + st["other_samples"]


def test_final48_has_no_overflow_and_its_hits_are_the_feature_passs():
    sph, cam = edge_inputs.golden_scene("final48")
    p = make_params(32, 18, 8, 50, 404)
    tab, st = mr.table(sph, cam, p, 8)
    check_invariant(tab)
    assert int(tab["used"].max()) <= 4 and st["overflow_pixels"] == 0 and st["other_samples"] == 0
    assert 1 < int(tab["used"].max())
    for n in (1, 5, 8):
        assert mr.table(sph, cam, p, n)[1]["hits"] == fsr.features(sph, cam, p, n)[2]["hits"]


def test_one_sample_is_the_first_segment_of_ray_color():
    sph, cam = edge_inputs.golden_scene("final48")
    sph = list(sph)
    p = make_params(16, 9, 2, 50, 404)
    tab, st = mr.table(sph, cam, p, 1)
    E = cast_ref.extent(sph)
    for y in range(9):
        for x in range(16):
            o, d, seed, skip = rr.camera_start(cam, p, y, x, 0)
            rec = rr.ray_color(sph, E, o, d, seed, skip)
            assert int(tab[y, x]["id"][0]) == rec["id_first"]  # (NO_ID is the sky's id)
            assert int(tab[y, x]["miss"]) == (rec["id_first"] == rr.NO_ID) and int(tab[y, x]["n"]) == 1
    assert rr.NO_ID == SKY and 0 < st["hits"] < 16 * 9


def test_own_counts_fold_each_pixels_first_samples():
    sph, cam = edge_inputs.golden_scene("final48")
    p = make_params(16, 9, 8, 50, 404)
    counts = np.full((9, 16), 4, np.uint32)
    counts[::2, 1::3] = 8
    counts[4, 5] = 0
    tab, st = mr.table(sph, cam, p, counts)
    t4, t8 = mr.table(sph, cam, p, 4)[0], mr.table(sph, cam, p, 8)[0]
    pick = np.where(counts == 8, t8, t4)
    pick[4, 5] = mr.table(sph, cam, p, 0)[0][4, 5]
    assert tab.tobytes() == pick.tobytes() and (tab["n"] == counts).all() and st["samples"] == int(counts.sum())
    assert int(tab[4, 5]["used"]) == 0 and (tab[4, 5]["id"] == SKY).all()


def test_coverage_of_a_hand_written_table():
    tab = np.zeros((1, 4), records.MATTE_DTYPE)
    for j, ids in enumerate(([3, 3, 5, -1], [-1, -1], [], list(range(10, 19)) + [3])):
        rec = mr.fold_ids(ids)
        for f in records.MATTE_DTYPE.names:
            tab[0, j][f] = rec[f]
    cov, grey, st = mr.coverage(tab, [3, 3])
    assert cov.tolist() == [[0.5, 0.0, 0.0, 0.0]] and grey.tolist() == [[128, 0, 0, 0]]
    assert st == dict(pixels_selected=1, pixels_uncertain=1, samples_selected=2)
    cov, grey, st = mr.coverage(tab, [SKY, 5, 3, 5])
    assert cov.tolist() == [[1.0, 1.0, 0.0, 0.0]] and grey.tolist() == [[255, 255, 0, 0]]  # (0.999 * 256 = 255.7)
    assert st == dict(pixels_selected=2, pixels_uncertain=1, samples_selected=6)
    cov, _, _ = mr.coverage(tab, [10, 17])
    assert cov[0, 3] == 2 / 10 and tab[0, 3]["other"] == 2  # (a lower bound: sphere 3 went to `other`)


def test_header_records_and_entry_points():
    header = open(os.path.join(ROOT, "include", "ykgpu.h")).read()
    for name in ("ykgpu_film_mattes", "ykgpu_film_matte_coverage", "ykgpu_group_film_mattes", "ykgpu_group_film_matte_coverage"):
        assert name in yk.EXPORTS and f"int {name}(" in header
    assert "typedef struct yk_matte_pixel { /* 80 bytes */" in header and "YK_MATTE_SKY = 0xFFFFFFFFu" in header
    assert ctypes.sizeof(records.MattePixel) == records.MATTE_DTYPE.itemsize == 80
    assert [records.MATTE_DTYPE.fields[f][1] for f in records.MATTE_DTYPE.names] == [0, 32, 64, 68, 72, 76]
    assert [getattr(records.MattePixel, f).offset for f in records.MATTE_DTYPE.names] == [0, 32, 64, 68, 72, 76]
    assert ctypes.sizeof(records.MatteStats) == 40 and records.MatteStats.overflow_pixels.offset == 32
    assert ctypes.sizeof(records.MatteCoverageStats) == 32
    lib = yk.load_library()
    assert lib.ykgpu_film_mattes(None, 0, None, None) == 1 and b"null film" in lib.ykgpu_last_error()
    assert lib.ykgpu_film_matte_coverage(None, None, 0, None, None, None) == 1
    assert lib.ykgpu_group_film_mattes(None, 0, None, None) == 1 and lib.ykgpu_group_film_matte_coverage(None, None, 0, None, None, None) == 1
    for cls in (yk.Film, yk.GroupFilm):
        assert hasattr(cls, "mattes") and hasattr(cls, "matte_coverage")
    assert lib.ykgpu_abi_version() == 11
