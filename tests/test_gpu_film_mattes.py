"""ykgpu_film_mattes and ykgpu_film_matte_coverage on the MI355X (include/ykgpu.h "film mattes",
DESIGN.md §6.10): the id-coverage table, its stats, the coverage and its grey image compared byte for
byte, every pixel, with the restatement of the definition (mattes_ref).  The shapes are the sampled
feature pass's smallest: a thin lens and a pinhole camera, n below, at and off the seed walk's four,
sizes that are no multiple of the 32 x 8 block, both engines and seed modes, a seed that wraps, a
strided tile, ties, negative radii, a scene of 700 spheres whose pixels overflow the 8 slots, the
ordered scan, the whole-engine redo, the film's own counts (uniform, adaptive, none), the table
cache beside the feature planes' cache, and a group of three entries over 17 rows.
"""
import ctypes
import os

import numpy as np
import pytest

import edge_inputs
import film_features_ref as ffr
import film_features_sampled_ref as fsr
import mattes_ref as mr
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd import records
from uecraytracing_amd.records import (FLAG_LINEAR_SCAN, MATTE_DTYPE, MATTE_SKY, PRECISION_FP32, RNG_XOR128,
                                       SEED_RANDOM_DEVICE, MatteCoverageStats, MatteStats, make_params)

pytestmark = pytest.mark.gpu

CAM = refscenes.reference_camera()
YK_ERR_INVALID = 1
KEY = 0x1234567890ABCDEF
LAZY = "YKGPU_FEATURE_LAZY_WORDS"
COUNTS = ("samples", "hits", "other_samples", "overflow_pixels")


@pytest.fixture(scope="module")
def ren():
    r = yk.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def final48():
    return edge_inputs.golden_scene("final48")


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check(film, scene, cam, p, n, what, ref_n=None):
    """film.mattes(n) against the yardstick at ref_n (n itself, or the film's counts)."""
    tab, st = film.mattes(n)
    want, wst = mr.table(scene, cam, p, n if ref_n is None else ref_n)
    bad = [f for f in MATTE_DTYPE.names if not (tab[f] == want[f]).all()]
    assert same(tab, want), f"table {what} n={n}: fields {bad} differ, {int((tab != want).sum())} of {want.size} pixels"
    assert {k: st[k] for k in COUNTS} == wst, what
    return tab, st


def check_coverage(film, tab, ids, what):
    cov, grey, st = film.matte_coverage(ids)
    wc, wg, wst = mr.coverage(tab, ids)
    assert same(cov, wc) and same(grey, wg), f"coverage {what}: {int((cov != wc).sum())} of {wc.size} pixels differ"
    assert {k: v for k, v in st.items() if k != "ms"} == wst and st["ms"] > 0, what
    return cov, grey, st


# ---- 1. the table against the yardstick ------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_final48_thin_lens(ren, final48, n):
    sph, cam = final48
    assert cam.lens_radius > 0
    ren.set_scene(sph, cam)
    p = make_params(32, 18, 8, 50, 404)
    with ren.film(p) as film:  # (an empty film: the first n samples need none rendered)
        tab, st = check(film, sph, cam, p, n, "final48")
        assert st["ms"] > 0 and st["redo_pixels"] == 0 and 0 < st["hits"] < st["samples"] == 32 * 18 * n
        assert st["overflow_pixels"] == 0 and (tab["n"] == n).all()
        sums, sumsq, done = film.read()
        assert not sums.any() and not sumsq.any() and done == 0 and not film.counts().any()  # (the film is untouched)


def test_many700_overflows_the_slots(ren):
    scene = ffr.many(700)
    ren.set_scene(scene, CAM)
    p = make_params(16, 9, 32, 50, 404)
    with ren.film(p) as film:
        tab, st = check(film, scene, CAM, p, 32, "many700")
        assert st["overflow_pixels"] > 0 and st["other_samples"] >= st["overflow_pixels"]
        assert int((tab["used"] == 8).sum()) > st["overflow_pixels"]  # (pixels with exactly 8 ids do not overflow)
        check_coverage(film, tab, [int(tab["id"][0, 0, 0]), 699, MATTE_SKY], "many700")


def test_ref4_pinhole_odd_size(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    p = make_params(33, 17, 4, 50, 404)
    with ren.film(p) as film:
        check(film, refscenes.ref4(), CAM, p, 3, "ref4 33x17")


@pytest.mark.parametrize("name", ["dupes", "shell"])
def test_ties_and_negative_radii(ren, name):
    scene = dict(dupes=refscenes.dupes, shell=ffr.shell)[name]()
    ren.set_scene(scene, CAM)
    p = make_params(16, 9, 4, 50, 404)
    with ren.film(p) as film:
        tab, _ = check(film, scene, CAM, p, 2, name)
    if name == "dupes":  # (of coincident spheres the last tuple index wins)
        assert (int(tab[4, 8]["id"][0]), int(tab[4, 8]["count"][0])) == (6, 2)


@pytest.mark.parametrize("kw", [dict(rng=RNG_XOR128), dict(seed_mode=SEED_RANDOM_DEVICE, seed_key=KEY), dict(seed0=4294967000)],
                         ids=["xor128", "keyed", "seed-wraps"])
def test_engines_and_seed_modes(ren, final48, kw):
    sph, cam = final48
    ren.set_scene(sph, cam)
    kw = dict(kw)
    p = make_params(32, 18, 8, 50, kw.pop("seed0", 404), **kw)
    with ren.film(p) as film:
        assert film.params.seed_key == p.seed_key
        check(film, sph, cam, p, 5, str(kw))


def test_strided_tile_linear_scan_and_fp32_film(ren, final48):
    sph, cam = final48
    ren.set_scene(sph, cam)
    whole_p = make_params(32, 18, 8, 50, 404)
    with ren.film(whole_p) as film:
        whole, wst = check(film, sph, cam, whole_p, 5, "whole")
    # rows 1, 4, 7, ... and column bands of 2, every 3rd
    tp = make_params(32, 18, 8, 50, 404, rows=(1, 6, 3), cols=(0, 12, 3, 1))
    with ren.film(tp) as film:
        got, _ = check(film, sph, cam, tp, 5, "strided")
    ys, xs = list(range(1, 18, 3)), [x for b in range(0, 32, 6) for x in (b, b + 1)]
    assert same(got, np.ascontiguousarray(whole[ys][:, xs]))
    for kw in (dict(flags=FLAG_LINEAR_SCAN), dict(precision=PRECISION_FP32)):
        with ren.film(make_params(32, 18, 8, 50, 404, **kw)) as film:
            tab, st = film.mattes(5)
            assert same(tab, whole) and {k: st[k] for k in COUNTS} == {k: wst[k] for k in COUNTS}, kw


# ---- 2. consistency with the render and the feature pass ---------------------------------------------

def test_one_sample_is_the_renders_first_hit(ren, final48):
    sph, cam = final48
    ren.set_scene(sph, cam)
    p = make_params(32, 18, 8, 50, 404)
    with ren.film(p) as film:
        tab, st = film.mattes(1)
        assert st["hits"] == film.features_sampled(1)[2]["hits"]
        assert film.mattes(5)[1]["hits"] == film.features_sampled(5)[2]["hits"]
    ys, xs = np.meshgrid(np.arange(18), np.arange(32), indexing="ij")
    rays = yk.camera_sample_rays(cam, p, ys.ravel(), xs.ravel(), np.zeros(ys.size, np.uint32))
    rec = ren.radiance_rays(rays).reshape(18, 32)
    assert records.NO_HIT_ID == MATTE_SKY
    assert same(np.ascontiguousarray(tab["id"][..., 0]), np.ascontiguousarray(rec["id_first"]))
    assert (tab["miss"] == (rec["id_first"] == MATTE_SKY)).all() and st["hits"] > 300


# ---- 3. the whole-engine redo ------------------------------------------------------------------------

def test_redo_path_gives_the_same_bytes(ren, final48):
    sph, cam = final48
    ren.set_scene(sph, cam)
    p = make_params(32, 18, 8, 50, 404)
    with ren.film(p) as film:
        plain, st = check(film, sph, cam, p, 8, "unforced")
        assert st["redo_pixels"] == 0
    assert LAZY not in os.environ
    os.environ[LAZY] = "8"  # the jitter's four words and one lens try: a second try goes to the redo
    try:
        with ren.film(p) as film:
            forced, fst = film.mattes(8)
    finally:
        del os.environ[LAZY]
    assert same(forced, plain) and 0 < fst["redo_pixels"] <= 32 * 18
    assert {k: fst[k] for k in COUNTS} == {k: st[k] for k in COUNTS}
    with ren.film(p) as film:  # (the limit was for that call alone)
        assert film.mattes(8)[1]["redo_pixels"] == 0


# ---- 4. the film's own counts -------------------------------------------------------------------------

def test_own_counts_of_a_uniform_an_adaptive_and_an_empty_film(ren, final48):
    sph, cam = final48
    ren.set_scene(sph, cam)
    p = make_params(32, 18, 16, 50, 404)
    with ren.film(p) as film:
        # no samples yet: n = 0 records, coverage 0.0
        tab, st = check(film, sph, cam, p, 0, "empty")
        assert not tab["n"].any() and (tab["id"] == MATTE_SKY).all() and st["samples"] == 0 and st["ms"] > 0
        cov, grey, cst = check_coverage(film, tab, [0, MATTE_SKY], "empty")
        assert not cov.any() and not grey.any() and cst["pixels_selected"] == 0
        # a uniform film: its `done`
        film.accumulate(3)
        own, st = check(film, sph, cam, p, 0, "uniform", ref_n=3)
        assert same(own, film.mattes(3)[0]) and (own["n"] == 3).all()
        film.accumulate(1)
        # an adaptive pass: counts 4 and 8, lanes of a wave with different trip counts
        e2, _ = film.error(0.0)
        film.accumulate_adaptive(float(np.median(e2)), 4)
        assert film.count_range() == (4, 8)
        counts = film.counts()
        sums = film.read()[0]
        own, st = check(film, sph, cam, p, 0, "adaptive", ref_n=counts)
        assert same(own["n"], counts) and st["samples"] == int(counts.sum()) and st["redo_pixels"] == 0
        assert same(film.counts(), counts) and same(film.read()[0], sums)  # (the film is untouched)
        check_coverage(film, own, [0, 1, MATTE_SKY], "adaptive")


# ---- 5. coverage --------------------------------------------------------------------------------------

def test_coverage_against_the_yardstick(ren, final48):
    sph, cam = final48
    ren.set_scene(sph, cam)
    p = make_params(32, 18, 8, 50, 404)
    with ren.film(p) as film:
        tab, _ = check(film, sph, cam, p, 8, "final48")
        present = sorted({int(k) for k in tab["id"].ravel() if k != MATTE_SKY})
        assert len(present) > 8
        cov, grey, st = check_coverage(film, tab, [present[0]], "one id")
        assert 0 < st["pixels_selected"] < 32 * 18 and st["pixels_uncertain"] == 0 and 0 < cov.max() <= 1.0
        assert len(np.unique(cov)) > 2  # (antialiased: partial coverage at the edges)
        some = [present[3], MATTE_SKY, present[1], present[3], present[-1]]  # (unsorted, with a duplicate)
        check_coverage(film, tab, some, "several ids and the sky")
        cov, grey, st = check_coverage(film, tab, present + [MATTE_SKY], "every id and the sky")
        assert (cov == 1.0).all() and (grey == 255).all() and st["samples_selected"] == 32 * 18 * 8
        sky, _, sst = check_coverage(film, tab, [MATTE_SKY], "the sky")
        spheres, _, pst = check_coverage(film, tab, present, "every id")
        assert sst["samples_selected"] + pst["samples_selected"] == 32 * 18 * 8
        only_cov, none, _ = film.matte_coverage([present[0]], want_grey=False)
        none2, only_grey, _ = film.matte_coverage([present[0]], want_cov=False)
        assert none is None and none2 is None
        assert same(only_cov, mr.coverage(tab, [present[0]])[0]) and same(only_grey, mr.coverage(tab, [present[0]])[1])


# ---- 6. the table cache -------------------------------------------------------------------------------

def test_cache_beside_the_feature_planes(ren, final48):
    sph, cam = final48
    ren.set_scene(sph, cam)
    p = make_params(32, 18, 8, 50, 404)
    with ren.film(p) as film:
        f0 = film.features_sampled(4)
        assert f0[2]["ms"] > 0
        a = check(film, sph, cam, p, 4, "first")
        assert a[1]["ms"] > 0
        b = check(film, sph, cam, p, 4, "again")
        assert b[1]["ms"] == 0.0 and {k: v for k, v in b[1].items() if k != "ms"} == {k: v for k, v in a[1].items() if k != "ms"}
        f1 = film.features_sampled(4)  # (the planes and their cache are the film's other buffer)
        assert f1[2]["ms"] == 0.0 and same(f1[0], f0[0]) and same(f1[1], f0[1])
        assert same(f1[0], fsr.features(sph, cam, p, 4)[0])
        c = check(film, sph, cam, p, 5, "another n")
        assert c[1]["ms"] > 0 and not same(c[0], a[0])
        film.accumulate(5)
        d = check(film, sph, cam, p, 5, "after accumulate")
        assert d[1]["ms"] == 0.0
        for again in range(2):  # (own counts always recompute)
            e = check(film, sph, cam, p, 0, "own counts", ref_n=5)
            assert e[1]["ms"] > 0 and same(e[0], c[0])
        assert film.mattes(5)[1]["ms"] > 0  # (the table is the own-counts pass's, whatever it counted)
        assert film._lib.ykgpu_film_mattes(film._f, 5, None, None) == 0  # (both outputs may be null)
        assert film.features_sampled(4)[2]["ms"] == 0.0


# ---- 7. errors ----------------------------------------------------------------------------------------

def test_refused_calls_write_nothing(ren, final48):
    sph, cam = final48
    ren.set_scene(sph, cam)
    p = make_params(32, 18, 8, 50, 404)
    sent_t = np.full((18, 32, 20), 0x77777777, np.uint32)
    sent_c = np.full((18, 32), -7.25)
    sent_g = np.full((18, 32), 77, np.uint8)
    nsph = len(sph)

    def matte_call(film, n):
        st = MatteStats(-1.0, 7, 7, 7, 7, 7)
        rc = film._lib.ykgpu_film_mattes(film._f, n, sent_t.ctypes.data, ctypes.byref(st))
        assert (sent_t == 0x77777777).all()
        assert (st.ms, st.samples, st.hits, st.other_samples, st.overflow_pixels, st.redo_pixels) == (-1.0, 7, 7, 7, 7, 7)
        return rc

    def cover_call(film, ids, n_ids=None, cov=True, grey=True):
        k = np.asarray(ids, np.uint32) if ids is not None else None
        st = MatteCoverageStats(-1.0, 7, 7, 7)
        rc = film._lib.ykgpu_film_matte_coverage(film._f, k.ctypes.data if k is not None else None,
                                                 len(k) if n_ids is None else n_ids, sent_c.ctypes.data if cov else None,
                                                 sent_g.ctypes.data if grey else None, ctypes.byref(st))
        assert (sent_c == -7.25).all() and (sent_g == 77).all()
        assert (st.ms, st.pixels_selected, st.pixels_uncertain, st.samples_selected) == (-1.0, 7, 7, 7)
        return rc

    with ren.film(p) as film:
        assert cover_call(film, [0]) == YK_ERR_INVALID and b"no matte table" in film._lib.ykgpu_last_error()
        assert matte_call(film, 9) == YK_ERR_INVALID and b"target" in film._lib.ykgpu_last_error()
        assert cover_call(film, [0]) == YK_ERR_INVALID  # (a refused pass leaves no table)
        tab, _ = film.mattes(4)
        assert cover_call(film, [0], n_ids=0) == YK_ERR_INVALID
        assert cover_call(film, None, n_ids=1) == YK_ERR_INVALID
        assert cover_call(film, [0, nsph]) == YK_ERR_INVALID and cover_call(film, [0xFFFFFFFE]) == YK_ERR_INVALID
        assert cover_call(film, [0], cov=False, grey=False) == YK_ERR_INVALID
        assert matte_call(film, 9) == YK_ERR_INVALID
        check_coverage(film, tab, [nsph - 1, MATTE_SKY], "after the refusals")  # (the table survived them)
        # a stale scene
        ren.set_scene(sph, cam)
        assert matte_call(film, 4) == YK_ERR_INVALID and b"scene" in film._lib.ykgpu_last_error()
        assert matte_call(film, 0) == YK_ERR_INVALID


# ---- 8. group films -----------------------------------------------------------------------------------

def test_group_film_gives_the_single_films_bytes(ren, final48):
    sph, cam = final48
    p = make_params(32, 17, 16, 50, 404)  # 17 rows over three entries: 6, 6, 5
    g = yk.Group([0, 0, 0])
    try:
        g.set_scene(sph, cam)
        ren.set_scene(sph, cam)
        with g.film(p) as gf, ren.film(p) as sf:
            sent, zero = np.full((17, 32), -7.25), np.zeros(1, np.uint32)
            assert gf._lib.ykgpu_group_film_matte_coverage(gf._f, zero.ctypes.data, 1, sent.ctypes.data, None,
                                                           None) == YK_ERR_INVALID and (sent == -7.25).all()  # (no table yet)
            gt, gst = check(gf, sph, cam, p, 4, "group")
            stt, sst = sf.mattes(4)
            assert same(gt, stt) and {k: gst[k] for k in COUNTS} == {k: sst[k] for k in COUNTS}
            assert gst["ms"] > 0 and gst["redo_pixels"] == 0 and gf.mattes(4)[1]["ms"] == 0.0
            ids = [int(gt["id"][8, 16, 0]), 0, MATTE_SKY]
            gc, sc = check_coverage(gf, gt, ids, "group"), sf.matte_coverage(ids)
            assert same(gc[0], sc[0]) and same(gc[1], sc[1])
            assert {k: v for k, v in gc[2].items() if k != "ms"} == {k: v for k, v in sc[2].items() if k != "ms"}
            assert gf.accumulate(4) == 4 == sf.accumulate(4)
            e2, _ = sf.error(0.0)
            thr = float(np.median(e2))
            gf.accumulate_adaptive(thr, 4)
            sf.accumulate_adaptive(thr, 4)
            assert gf.count_range() == sf.count_range() == (4, 8)
            go, gost = check(gf, sph, cam, p, 0, "group own counts", ref_n=sf.counts())
            assert same(go, sf.mattes(0)[0]) and gost["samples"] == int(sf.counts().sum())
            tsent = np.full((17, 32, 20), 0x77777777, np.uint32)
            assert gf._lib.ykgpu_group_film_mattes(gf._f, 17, tsent.ctypes.data, None) == YK_ERR_INVALID
            assert (tsent == 0x77777777).all()
    finally:
        g.close()
