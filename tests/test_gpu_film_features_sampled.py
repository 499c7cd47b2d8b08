"""ykgpu_film_features_sampled and ykgpu_film_denoise_guided_sampled on the MI355X (include/ykgpu.h
"sampled film features"): the feature means and variances, the guided mean and its
RGB8 image compared byte for byte, every pixel, with the numpy restatement of the definition
(film_features_sampled_ref).  The shapes are the smallest at which each path of the kernels is taken:
a thin lens and a pinhole camera, n below, at and off the seed walk's four, sizes that are no multiple
of the 32 x 8 block, both engines and seed modes, a seed that wraps, a strided tile, ties, negative
radii, a scene of 700 spheres, the ordered scan, the whole-engine redo (the lazy-word limit lowered),
the plane cache against the pinhole pass, and a group of three entries over 17 rows.
"""
import ctypes
import os

import numpy as np
import pytest

import edge_inputs
import film_denoise_ref as fdr
import film_features_ref as ffr
import film_features_sampled_ref as fsr
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd import records
from uecraytracing_amd.records import (FLAG_LINEAR_SCAN, PRECISION_FP32, RNG_XOR128, SEED_RANDOM_DEVICE, DenoiseParams,
                                       FeatureParams, GroupDenoiseStats, GuidedStats, SampledFeaturesStats, make_params)

pytestmark = pytest.mark.gpu

CAM = refscenes.reference_camera()
YK_ERR_INVALID, YK_ERR_UNSUPPORTED = 1, 4
INF = float("inf")
KEY = 0x1234567890ABCDEF
LAZY = "YKGPU_FEATURE_LAZY_WORDS"


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


def check(film, scene, cam, p, n, what):
    mean, var, st = film.features_sampled(n)
    F, U, want = fsr.features(scene, cam, p, n)
    assert same(mean, F), f"mean {what} n={n}: {int((mean != F).sum())} of {F.size} values differ"
    assert same(var, U), f"variance {what} n={n}: {int((var != U).sum())} of {U.size} values differ"
    assert (st["samples"], st["hits"]) == (want["samples"], want["hits"]), what
    return mean, var, st


# ---- 1. the planes against the yardstick -----------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_final48_thin_lens(ren, final48, n):
    sph, cam = final48
    assert cam.lens_radius > 0
    ren.set_scene(sph, cam)
    p = make_params(32, 18, 8, 50, 404)
    with ren.film(p) as film:  # (an empty film: the features need no samples)
        _, var, st = check(film, sph, cam, p, n, "final48")
        assert st["ms"] > 0 and st["redo_pixels"] == 0 and 0 < st["hits"] < st["samples"]
        assert var.any() == (n > 1)
        sums, sumsq, done = film.read()
        assert not sums.any() and not sumsq.any() and done == 0  # (the film is untouched)


def test_ref4_pinhole_odd_size(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    p = make_params(33, 17, 4, 50, 404)
    with ren.film(p) as film:
        check(film, refscenes.ref4(), CAM, p, 3, "ref4 33x17")


@pytest.mark.parametrize("name", ["dupes", "shell", "many700"])
def test_ties_negative_radii_and_a_large_scene(ren, name):
    scene = dict(dupes=refscenes.dupes, shell=ffr.shell, many700=lambda: ffr.many(700))[name]()
    ren.set_scene(scene, CAM)
    p = make_params(16, 9, 4, 50, 404)
    with ren.film(p) as film:
        mean, _, _ = check(film, scene, CAM, p, 2, name)
    if name == "dupes":  # (of coincident spheres the last tuple index wins)
        assert tuple(mean[4, 8, 0:3]) == tuple(refscenes.dupes()[6].albedo)
    if name == "many700":  # (the last index of the table)
        assert tuple(mean[4, 8, 0:3]) == (0.25, 0.5, 0.75)


@pytest.mark.parametrize("kw", [dict(rng=RNG_XOR128), dict(seed_mode=SEED_RANDOM_DEVICE, seed_key=KEY),
                                dict(rng=RNG_XOR128, seed_mode=SEED_RANDOM_DEVICE, seed_key=KEY), dict(seed0=4294967000)],
                         ids=["xor128", "keyed", "xor128-keyed", "seed-wraps"])
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
        whole, wvar, _ = check(film, sph, cam, whole_p, 5, "whole")
    # rows 1, 4, 7, ... and column bands of 2, every 3rd
    tp = make_params(32, 18, 8, 50, 404, rows=(1, 6, 3), cols=(0, 12, 3, 1))
    with ren.film(tp) as film:
        got, gvar, _ = check(film, sph, cam, tp, 5, "strided")
    ys, xs = list(range(1, 18, 3)), [x for b in range(0, 32, 6) for x in (b, b + 1)]
    assert same(got, np.ascontiguousarray(whole[ys][:, xs])) and same(gvar, np.ascontiguousarray(wvar[ys][:, xs]))
    with ren.film(make_params(32, 18, 8, 50, 404, flags=FLAG_LINEAR_SCAN)) as film:
        m, v, st = film.features_sampled(5)
        assert same(m, whole) and same(v, wvar) and st["redo_pixels"] == 0
    with ren.film(make_params(32, 18, 8, 50, 404, precision=PRECISION_FP32)) as film:
        m, v, _ = film.features_sampled(5)
        assert same(m, whole) and same(v, wvar)


# ---- 2. consistency with the render -----------------------------------------------------------------

def test_one_sample_is_the_renders_first_segment(ren, final48):
    sph, cam = final48
    ren.set_scene(sph, cam)
    p = make_params(32, 18, 8, 50, 404)
    with ren.film(p) as film:
        F, _, _ = film.features_sampled(1)
    ys, xs = np.meshgrid(np.arange(18), np.arange(32), indexing="ij")
    rays = yk.camera_sample_rays(cam, p, ys.ravel(), xs.ravel(), np.zeros(ys.size, np.uint32))
    rec = ren.radiance_rays(rays).reshape(18, 32)
    assert same(np.ascontiguousarray(F[..., 6]), np.ascontiguousarray(rec["t_first"]))
    alb = np.ones((18, 32, 3))
    for i in range(18):
        for j in range(32):
            k = int(rec["id_first"][i, j])
            if k != records.NO_HIT_ID and sph[k].material != records.MATERIAL_DIELECTRIC:
                alb[i, j] = tuple(sph[k].albedo)
    assert same(np.ascontiguousarray(F[..., 0:3]), alb)
    assert (rec["id_first"] != records.NO_HIT_ID).sum() > 300


# ---- 3. the whole-engine redo ------------------------------------------------------------------------

def test_redo_path_gives_the_same_bytes(ren, final48):
    sph, cam = final48
    ren.set_scene(sph, cam)
    p = make_params(32, 18, 8, 50, 404)
    with ren.film(p) as film:
        plain, pvar, st = check(film, sph, cam, p, 8, "unforced")
        assert st["redo_pixels"] == 0
    assert LAZY not in os.environ
    os.environ[LAZY] = "8"  # the jitter's four words and one lens try: a second try goes to the redo
    try:
        with ren.film(p) as film:
            forced, fvar, st = film.features_sampled(8)
    finally:
        del os.environ[LAZY]
    assert same(forced, plain) and same(fvar, pvar)
    assert 0 < st["redo_pixels"] <= 32 * 18 and (st["samples"], st["hits"]) == (32 * 18 * 8, int(fsr.features(sph, cam, p, 8)[2]["hits"]))
    with ren.film(p) as film:  # (the limit was for that call alone)
        assert film.features_sampled(8)[2]["redo_pixels"] == 0


# ---- 4. the plane cache ------------------------------------------------------------------------------

def test_cache_and_the_pinhole_pass(ren, final48):
    sph, cam = final48
    ren.set_scene(sph, cam)
    p = make_params(32, 18, 8, 50, 404)
    with ren.film(p) as film:
        pin0 = film.features(2)
        assert pin0[2] > 0
        a = check(film, sph, cam, p, 4, "first")
        assert a[2]["ms"] > 0
        b = check(film, sph, cam, p, 4, "again")
        assert b[2]["ms"] == 0.0 and {k: v for k, v in b[2].items() if k != "ms"} == {k: v for k, v in a[2].items() if k != "ms"}
        film.accumulate(3)
        c = check(film, sph, cam, p, 4, "after accumulate")
        assert c[2]["ms"] == 0.0
        pin1 = film.features(2)  # (either kind replaces the other)
        assert pin1[2] > 0 and same(pin1[0], pin0[0]) and same(pin1[1], pin0[1])
        F, U = ffr.features(sph, cam, p, 2)
        assert same(pin1[0], F) and same(pin1[1], U)
        assert film.features(2)[2] == 0.0
        d = check(film, sph, cam, p, 4, "after the pinhole pass")
        assert d[2]["ms"] > 0
        e = check(film, sph, cam, p, 5, "another n")
        assert e[2]["ms"] > 0 and not same(e[0], d[0])
        lib, f = film._lib, film._f
        only = np.full((18, 32, 7), -7.25)
        assert lib.ykgpu_film_features_sampled(f, 5, None, only.ctypes.data, None) == 0 and same(only, e[1])
        assert lib.ykgpu_film_features_sampled(f, 5, None, None, None) == 0


# ---- 5. the guided filter ----------------------------------------------------------------------------

def guided_ref(film, scene, cam, p, n, colour=None, feat=None):
    sums, sumsq, _ = film.read()
    return fsr.denoise_guided(sums, sumsq, film.counts(), scene, cam, p, n, colour=colour, feat=feat)


def test_guided_sampled_against_the_yardstick(ren, final48):
    sph, cam = final48
    ren.set_scene(sph, cam)
    p = make_params(32, 18, 16, 50, 404)
    dp0, fp0, n0 = yk.guided_sampled_defaults()
    with ren.film(p) as film:
        film.accumulate(8)
        mean, rgb, st = film.denoise_guided_sampled()
        want = guided_ref(film, sph, cam, p, n0)
        assert same(mean, want) and same(rgb, fdr.to_rgb8(want))
        assert st["features_ms"] > 0 and film.denoise_guided_sampled()[2]["features_ms"] == 0.0
        assert same(film.features_sampled(n0)[0], fsr.features(sph, cam, p, n0)[0])
        # R = 2, F = 1, another n, and a grid that the pinhole call would refuse
        dp = DenoiseParams(2, 1, dp0.k2, dp0.alpha, dp0.eps)
        fp = FeatureParams(9, 0, fp0.k2, fp0.alpha, fp0.tau_albedo, fp0.tau_normal, fp0.tau_depth)
        mean, rgb, _ = film.denoise_guided_sampled(dp, fp, 8)
        want = guided_ref(film, sph, cam, p, 8, colour=dict(radius=2, patch=1))
        assert same(mean, want) and same(rgb, fdr.to_rgb8(want))
        only_mean, none, _ = film.denoise_guided_sampled(dp, fp, 8, want_rgb=False)
        assert none is None and same(only_mean, want)
        # every group off: the colour-only filter
        off = FeatureParams(2, 0, fp0.k2, fp0.alpha, INF, INF, INF)
        m_off, r_off, _ = film.denoise_guided_sampled(dp0, off, 8)
        m_col, r_col, _ = film.denoise(dp0.radius, dp0.patch, dp0.k2, dp0.alpha, dp0.eps)
        assert same(m_off, m_col) and same(r_off, r_col)
        # the pinhole guided call still returns its own bytes
        pm, _, _ = film.denoise_guided()
        sums, sumsq, _ = film.read()
        assert same(pm, ffr.denoise_guided(sums, sumsq, 8, sph, cam, p))


def test_guided_sampled_on_an_adaptive_film(ren, final48):
    sph, cam = final48
    ren.set_scene(sph, cam)
    p = make_params(32, 18, 16, 50, 404)
    with ren.film(p) as film:
        film.accumulate(4)
        e2, _ = film.error(0.0)
        film.accumulate_adaptive(float(np.median(e2)), 4)
        lo, hi = film.count_range()
        assert (lo, hi) == (4, 8)
        mean, rgb, _ = film.denoise_guided_sampled(n_samples=4)
        want = guided_ref(film, sph, cam, p, 4)
        assert same(mean, want) and same(rgb, fdr.to_rgb8(want))


# ---- 6. errors ---------------------------------------------------------------------------------------

def test_refused_calls_write_nothing(ren, final48):
    sph, cam = final48
    ren.set_scene(sph, cam)
    p = make_params(32, 18, 8, 50, 404)
    sent7 = np.full((18, 32, 7), -7.25)
    sent3 = np.full((18, 32, 3), -7.25)
    sent8 = np.full((18, 32, 3), 77, np.uint8)

    def feat_call(film, n):
        st = SampledFeaturesStats(-1.0, 7, 7, 7, 7)
        rc = film._lib.ykgpu_film_features_sampled(film._f, n, sent7.ctypes.data, sent7.ctypes.data, ctypes.byref(st))
        assert (sent7 == -7.25).all() and (st.ms, st.samples, st.hits, st.redo_pixels) == (-1.0, 7, 7, 7)
        return rc

    def guided_call(film, n, dp=None, fp=None, mean=True, rgb=True):
        st = GuidedStats(-1.0, -1.0, -1.0, -1.0)
        rc = film._lib.ykgpu_film_denoise_guided_sampled(
            film._f, ctypes.byref(dp) if dp is not None else None, ctypes.byref(fp) if fp is not None else None, n,
            sent3.ctypes.data if mean else None, sent8.ctypes.data if rgb else None, ctypes.byref(st))
        assert (sent3 == -7.25).all() and (sent8 == 77).all() and st.total_ms == -1.0 and st.features_ms == -1.0
        return rc

    dp0, fp0, _ = yk.guided_sampled_defaults()
    with ren.film(p) as film:
        for bad in (0, 257, 9):  # (9: past the film's target of 8)
            assert feat_call(film, bad) == YK_ERR_INVALID
            assert guided_call(film, bad) == YK_ERR_INVALID
        assert guided_call(film, 4) == YK_ERR_INVALID  # no samples yet: a count below 2
        film.accumulate(1)
        assert guided_call(film, 4) == YK_ERR_INVALID
        film.accumulate(1)
        assert guided_call(film, 4, mean=False, rgb=False) == YK_ERR_INVALID  # both outputs NULL
        for fp in (FeatureParams(2, 1, 2.0, 1.0, 1e-2, 1e-1, 1e-2), FeatureParams(2, 0, 0.0, 1.0, 1e-2, 1e-1, 1e-2),
                   FeatureParams(2, 0, 2.0, -1.0, 1e-2, 1e-1, 1e-2), FeatureParams(2, 0, 2.0, 1.0, 0.0, 1e-1, 1e-2),
                   FeatureParams(2, 0, 2.0, 1.0, 1e-2, 1e-1, float("nan"))):
            assert guided_call(film, 4, fp=fp) == YK_ERR_INVALID
        for dp in (DenoiseParams(11, 1, 2.0, 1.0, 1e-10), DenoiseParams(5, 4, 2.0, 1.0, 1e-10),
                   DenoiseParams(5, 1, 0.0, 1.0, 1e-10)):
            assert guided_call(film, 4, dp=dp) == YK_ERR_INVALID
        sent3[:] = 0.0  # (a call that succeeds does write)
        sent8[:] = 0
        assert film._lib.ykgpu_film_denoise_guided_sampled(film._f, None, None, 4, sent3.ctypes.data, sent8.ctypes.data, None) == 0
        assert sent3.any() and sent8.any()
        sent3[:], sent8[:] = -7.25, 77
        # a stale scene
        ren.set_scene(sph, cam)
        assert feat_call(film, 4) == YK_ERR_INVALID and b"scene" in film._lib.ykgpu_last_error()
        assert guided_call(film, 4) == YK_ERR_INVALID
    # a strided tile: the pass works, the filter does not
    tp = make_params(32, 18, 8, 50, 404, rows=(1, 6, 3))
    with ren.film(tp) as film:
        film.accumulate(2)
        st = GuidedStats(-1.0, -1.0, -1.0, -1.0)
        m, r = np.full((6, 32, 3), -7.25), np.full((6, 32, 3), 77, np.uint8)
        assert film._lib.ykgpu_film_denoise_guided_sampled(film._f, None, None, 2, m.ctypes.data, r.ctypes.data,
                                                           ctypes.byref(st)) == YK_ERR_UNSUPPORTED
        assert (m == -7.25).all() and (r == 77).all() and st.total_ms == -1.0
        assert film.features_sampled(2)[2]["samples"] == 6 * 32 * 2


# ---- 7. group films ----------------------------------------------------------------------------------

def test_group_film_gives_the_single_films_bytes(ren, final48):
    sph, cam = final48
    p = make_params(32, 17, 16, 50, 404)  # 17 rows over three entries: 6, 6, 5
    g = yk.Group([0, 0, 0])
    try:
        g.set_scene(sph, cam)
        ren.set_scene(sph, cam)
        with g.film(p) as gf, ren.film(p) as sf:
            gm, gv, gst = gf.features_sampled(4)
            sm, sv, sst = sf.features_sampled(4)
            F, U, want = fsr.features(sph, cam, p, 4)
            assert same(gm, sm) and same(gv, sv) and same(gm, F) and same(gv, U)
            assert (gst["samples"], gst["hits"], gst["redo_pixels"]) == (sst["samples"], sst["hits"], 0)
            assert gst["samples"] == want["samples"] and gst["ms"] > 0
            gm2, gv2, gst2 = gf.features_sampled(4)
            assert same(gm2, sm) and same(gv2, sv) and gst2["ms"] == 0.0 and gst2["hits"] == sst["hits"]
            assert gf.accumulate(4) == 4 == sf.accumulate(4)
            for again in (False, True):
                a, b = gf.denoise_guided_sampled(n_samples=4), sf.denoise_guided_sampled(n_samples=4)
                assert same(a[0], b[0]) and same(a[1], b[1])
                assert isinstance(a[2], dict) and "exchange_ms" in a[2]
                assert (a[2]["features_ms"] == 0.0) == again
            e2, _ = sf.error(0.0)
            thr = float(np.median(e2))
            gf.accumulate_adaptive(thr, 4)
            sf.accumulate_adaptive(thr, 4)
            assert gf.count_range() == sf.count_range() == (4, 8) and same(gf.counts(), sf.counts())
            a, b = gf.denoise_guided_sampled(n_samples=4), sf.denoise_guided_sampled(n_samples=4)
            assert same(a[0], b[0]) and same(a[1], b[1])
            assert same(gf.features_sampled(4)[0], sm)
            # the group's own checks
            sent = np.full((17, 32, 7), -7.25)
            for bad in (0, 257, 17):
                assert gf._lib.ykgpu_group_film_features_sampled(gf._f, bad, sent.ctypes.data, sent.ctypes.data, None) == YK_ERR_INVALID
                st = GroupDenoiseStats()
                out = np.full((17, 32, 3), -7.25)
                assert gf._lib.ykgpu_group_film_denoise_guided_sampled(gf._f, None, None, bad, out.ctypes.data, None,
                                                                       ctypes.byref(st)) == YK_ERR_INVALID
                assert (sent == -7.25).all() and (out == -7.25).all()
    finally:
        g.close()
