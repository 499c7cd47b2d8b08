"""ykgpu_film_features and ykgpu_film_denoise_guided on the MI355X (include/ykgpu.h "film features"):
the feature means and variances, the guided mean and its RGB8 image compared byte for byte, with no
tolerance, with the numpy restatement of the definition (film_features_ref); the film's state read
back afterwards and asserted unchanged.  The shapes are the smallest at which each path of the
kernels is taken: every grid, sizes that are no multiple of the 32 x 8 block, sub-tiles and strided
tiles (features are per pixel in image coordinates), scenes that cross the feature kernel's 512-sphere
LDS chunk, a window that crosses every edge, a halo larger than the image, several blocks, per-pixel
counts and zero variance.  The guided filter has one layout (features from global memory), so every
(R, F) takes the same path.
"""
import ctypes

import numpy as np
import pytest

import film_adaptive_ref as far
import film_denoise_ref as fdr
import film_features_ref as ffr
import film_ref
import golden_data
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd.records import (PRECISION_FP32, RNG_XOR128, D3, Camera, DenoiseParams, FeatureParams,
                                       GuidedStats, make_params)

pytestmark = pytest.mark.gpu

CAM = refscenes.reference_camera()
REF4_20 = dict(width=16, height=9, spp=20, max_depth=50, seed0=404)
YK_ERR_INVALID, YK_ERR_UNSUPPORTED = 1, 4
INF = float("inf")
CHUNK = 512  # yk_features.hip kChunk


@pytest.fixture(scope="module")
def ren():
    r = yk.Renderer(0)
    yield r
    r.close()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_features(film, scene, cam, p, grid, what):
    mean, var, ms = film.features(grid)
    F, U = ffr.features(scene, cam, p, grid)
    assert same(mean, F), f"mean {what} g={grid}: {int((mean != F).sum())} of {F.size} values differ"
    assert same(var, U), f"variance {what} g={grid}: {int((var != U).sum())} of {U.size} values differ"
    return mean, var, ms


# ---- the feature pass ---------------------------------------------------------------------------

@pytest.mark.parametrize("grid", [1, 2, 4])
def test_features_ref4(ren, grid):
    p = make_params(**REF4_20)
    ren.set_scene(refscenes.ref4(), CAM)
    with ren.film(p) as film:  # (an empty film: the features need no samples)
        _, _, ms = check_features(film, refscenes.ref4(), CAM, p, grid, "ref4")
        assert ms > 0
        mean, var, ms2 = check_features(film, refscenes.ref4(), CAM, p, grid, "ref4 again")
        assert ms2 == 0.0  # the cached pass
        lib, f = film._lib, film._f
        only = np.full((9, 16, 7), -7.25)
        assert lib.ykgpu_film_features(f, grid, None, only.ctypes.data, None) == 0 and same(only, var)
        assert lib.ykgpu_film_features(f, grid, None, None, None) == 0
        other = 1 if grid != 1 else 2
        _, _, ms3 = check_features(film, refscenes.ref4(), CAM, p, other, "ref4 other grid")
        assert ms3 > 0
        # refused calls write nothing
        sent = np.full((9, 16, 7), -7.25)
        t = ctypes.c_double(-1.0)
        for bad in (0, 5):
            assert lib.ykgpu_film_features(f, bad, sent.ctypes.data, sent.ctypes.data, ctypes.byref(t)) == YK_ERR_INVALID
            assert (sent == -7.25).all() and t.value == -1.0
        sums, sumsq, done = film.read()
        assert not sums.any() and not sumsq.any() and done == 0 and not film.counts().any()  # (the film is untouched)


def test_features_odd_size_sub_tile_and_strided_tiles(ren):
    ren.set_scene(refscenes.mixed12(), CAM)
    scene = refscenes.mixed12()
    p = make_params(37, 20, 8, 50, 404)
    with ren.film(p) as film:
        whole, wvar, _ = check_features(film, scene, CAM, p, 2, "37x20")
    sub = make_params(37, 20, 8, 50, 404, rows=(3, 12, 1), cols=(5, 26, 1))
    with ren.film(sub) as film:
        part, pvar, _ = check_features(film, scene, CAM, sub, 2, "sub-tile")
    assert same(part, np.ascontiguousarray(whole[3:15, 5:31])) and same(pvar, np.ascontiguousarray(wvar[3:15, 5:31]))
    for kw, sl in ((dict(rows=(1, 9, 2)), (slice(1, 19, 2), slice(None))),
                   (dict(cols=(3, 11, 3)), (slice(None), slice(3, 36, 3))),
                   (dict(rows=(0, 8, 2, 1), cols=(2, 8, 2, 2)), None)):
        tp = make_params(37, 20, 8, 50, 404, **kw)
        with ren.film(tp) as film:
            got, _, _ = check_features(film, scene, CAM, tp, 2, f"strided {kw}")
        if sl is not None:
            assert same(got, np.ascontiguousarray(whole[sl]))
        else:
            ys, xs = film_ref.tile_rows(tp), film_ref.tile_cols(tp)
            assert same(got, np.ascontiguousarray(whole[ys][:, xs]))


def test_features_fp32_xor128_film_gives_the_fp64_bytes(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    p32 = make_params(**REF4_20, precision=PRECISION_FP32, rng=RNG_XOR128)
    with ren.film(p32) as film:
        check_features(film, refscenes.ref4(), CAM, make_params(**REF4_20), 2, "fp32 film")


@pytest.mark.parametrize("n", [CHUNK + 1, 700])
def test_features_scene_larger_than_the_lds_chunk(ren, n):
    scene = ffr.many(n)
    ren.set_scene(scene, CAM)
    p = make_params(**REF4_20)
    with ren.film(p) as film:
        mean, _, _ = check_features(film, scene, CAM, p, 2, f"{n} spheres")
        check_features(film, scene, CAM, p, 1, f"{n} spheres")
    assert tuple(mean[4, 8, 0:3]) == (0.25, 0.5, 0.75)  # the last index, from the second chunk


def test_features_coincident_spheres_shell_and_lens(ren):
    p = make_params(**REF4_20)
    ren.set_scene(refscenes.dupes(), CAM)
    with ren.film(p) as film:
        mean, _, _ = check_features(film, refscenes.dupes(), CAM, p, 2, "dupes")
    assert tuple(mean[4, 8, 0:3]) == tuple(refscenes.dupes()[6].albedo)
    ren.set_scene(ffr.shell(), CAM)
    with ren.film(p) as film:
        check_features(film, ffr.shell(), CAM, p, 2, "shell")
    lens = Camera(CAM.origin, CAM.lower_left_corner, CAM.horizontal, CAM.vertical, D3(1, 0, 0), D3(0, 1, 0), 0.25)
    ren.set_scene(refscenes.mixed12(), lens)
    with ren.film(p) as film:
        got, _, _ = check_features(film, refscenes.mixed12(), lens, p, 2, "thin lens")
    assert same(got, ffr.features(refscenes.mixed12(), CAM, p, 2)[0])


def test_features_refuse_a_stale_scene(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    with ren.film(make_params(**REF4_20)) as film:
        film.accumulate(4)
        film.features(2)
        ren.set_scene(refscenes.lambert3(), CAM)
        with pytest.raises(yk.YkError, match="YK_ERR_INVALID.*scene"):
            film.features(2)
        with pytest.raises(yk.YkError, match="YK_ERR_INVALID.*scene"):
            film.denoise_guided()


# ---- the guided filter --------------------------------------------------------------------------

def params_of(colour=None, feat=None):
    c = {**ffr.COLOUR_DEFAULTS, **(colour or {})}
    f = {**ffr.FEATURE_DEFAULTS, **(feat or {})}
    return (DenoiseParams(c["radius"], c["patch"], c["k2"], c["alpha"], c["eps"]),
            FeatureParams(f["grid"], 0, f["k2"], f["alpha"], f["tau_albedo"], f["tau_normal"], f["tau_depth"]))


def check(film, scene, cam, p, sums, sumsq, counts, what, colour=None, feat=None):
    """One guided denoise against the yardstick on the state (sums, sumsq, counts) the film must hold."""
    before = film.read() + (film.counts(),)
    assert same(before[0], sums) and same(before[1], sumsq), f"the film's state {what}"
    dp, fp = params_of(colour, feat)
    mean, rgb, st = film.denoise_guided(dp, fp)
    want = ffr.denoise_guided(sums, sumsq, counts, scene, cam, p, colour=colour, feat=feat)
    assert same(mean, want), f"mean {what}: {int((mean != want).sum())} of {want.size} values differ"
    assert same(rgb, fdr.to_rgb8(want)), f"rgb {what}"
    assert st["moments_ms"] >= 0 and st["filter_ms"] > 0 and st["total_ms"] >= st["filter_ms"] and st["features_ms"] >= 0
    after = film.read() + (film.counts(),)
    assert all(same(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(before, after)), f"state {what}"
    return mean, rgb, st


@pytest.mark.parametrize("colour", [None, dict(radius=1, patch=0), dict(radius=10, patch=3)],
                         ids=["defaults", "r1-f0", "r10-f3"])
def test_guided_ref4_after_chunks_of_4_and_16(ren, colour):
    p = make_params(**REF4_20)
    scene = refscenes.ref4()
    ren.set_scene(scene, CAM)
    S, Q = film_ref.prefixes(film_ref.colours(scene, CAM, p))
    with ren.film(p) as film:
        film.accumulate(4)
        _, _, st = check(film, scene, CAM, p, S[4], Q[4], 4, "after 4", colour=colour)
        assert st["features_ms"] > 0  # the first call computes the pass
        film.accumulate(16)
        mean, rgb, st = check(film, scene, CAM, p, S[20], Q[20], 20, "after 20", colour=colour)
        assert st["features_ms"] == 0.0  # ... and the film keeps it
        dp, fp = params_of(colour)
        only_mean, none, _ = film.denoise_guided(dp, fp, want_rgb=False)
        none2, only_rgb, _ = film.denoise_guided(dp, fp, want_mean=False)
        assert none is None and none2 is None and same(only_mean, mean) and same(only_rgb, rgb)
        if colour is None:  # NULL parameters are the defaults
            m0, r0, _ = film.denoise_guided()
            assert same(m0, mean) and same(r0, rgb)
            assert not same(mean, film.denoise(**ffr.COLOUR_DEFAULTS)[0])  # (the features bound the weight)
        # a grid of 1 and a switched-off group are other weights
        check(film, scene, CAM, p, S[20], Q[20], 20, "g=1, depth off", colour=colour, feat=dict(grid=1, tau_depth=INF))
        assert film.accumulate_adaptive(-1.0, 1).pixels_selected == 0  # (complete, and still usable)


def test_guided_all_groups_off_is_film_denoise(ren):
    p = make_params(**REF4_20)
    ren.set_scene(refscenes.ref4(), CAM)
    off = dict(tau_albedo=INF, tau_normal=INF, tau_depth=INF)
    with ren.film(p) as film:
        film.accumulate(8)
        for colour in (dict(fdr.DEFAULTS), dict(fdr.DEFAULTS, radius=10, patch=3), dict(fdr.DEFAULTS, radius=2, patch=0, k2=0.25)):
            mean, rgb, _ = film.denoise_guided(*params_of(colour, off))
            want_mean, want_rgb, _ = film.denoise(**colour)
            assert same(mean, want_mean) and same(rgb, want_rgb), colour


def test_guided_sizes_that_are_no_multiple_of_a_block_and_a_sub_tile(ren):
    scene = refscenes.ref4()
    ren.set_scene(scene, CAM)
    p = make_params(37, 20, 8, 50, 404)
    S, Q = film_ref.prefixes(film_ref.colours(scene, CAM, p))
    with ren.film(p) as film:
        film.accumulate(8)
        whole, _, _ = check(film, scene, CAM, p, S[8], Q[8], 8, "37x20")
    sub = make_params(37, 20, 8, 50, 404, rows=(3, 12, 1), cols=(5, 26, 1))
    with ren.film(sub) as film:
        film.accumulate(8)
        s, q = np.ascontiguousarray(S[8][3:15, 5:31]), np.ascontiguousarray(Q[8][3:15, 5:31])
        part, _, _ = check(film, scene, CAM, sub, s, q, 8, "sub-tile")
    assert part.shape == (12, 26, 3) and not same(part, np.ascontiguousarray(whole[3:15, 5:31]))


def test_guided_mixed12_several_blocks_and_it_beats_colour_only(ren):
    scene = refscenes.mixed12()
    ren.set_scene(scene, CAM)
    p = make_params(64, 36, 16, 50, 404)
    S, Q = film_ref.prefixes(film_ref.colours(scene, CAM, p))
    with ren.film(p) as film:
        film.accumulate(16)
        mean, _, _ = check(film, scene, CAM, p, S[16], Q[16], 16, "mixed12 64x36")
        base, _, _ = film.denoise()
    truth = fdr.truth(scene, CAM, 64, 36)
    guided, colour_only = fdr.mse(mean, truth), fdr.mse(base, truth)
    print("mixed12 64x36x16: colour-only", repr(colour_only), "guided", repr(guided), "ratio", guided / colour_only)
    assert guided < colour_only


def adaptive(ren, p, zero_variance=False):
    scene = refscenes.ref4()
    ren.set_scene(scene, CAM)
    sim = far.Sim(film_ref.colours(scene, CAM, p))
    p64 = make_params(**REF4_20)  # (the features are the FP64 pass whatever the film's precision)
    spreads = []
    with ren.film(p) as film:
        for i, (q, n) in enumerate(far.PASSES_A):
            thr2 = sim.threshold2(q)
            film.accumulate_adaptive(thr2, n)
            sim.step(thr2, n)
            assert same(film.counts(), sim.counts) and int(sim.counts.min()) >= 2
            spreads.append((int(sim.counts.min()), int(sim.counts.max())))
            if zero_variance and i == 0:
                _, v = fdr.moments(sim.sums(), sim.sumsq(), sim.counts)
                assert int((v.max(axis=2) == 0.0).sum()) > 0  # (the precondition: pixels on the eps path)
            check(film, scene, CAM, p64, sim.sums(), sim.sumsq(), sim.counts, f"after pass {i}")
    assert any(lo != hi for lo, hi in spreads), spreads  # (a non-uniform film was filtered)


def test_guided_non_uniform_film(ren):
    adaptive(ren, make_params(**REF4_20))


def test_guided_zero_variance_pixels_fp32_xor128(ren):
    adaptive(ren, make_params(**REF4_20, precision=PRECISION_FP32, rng=RNG_XOR128), zero_variance=True)


def raw_guided(film, dp=None, fp=None, want_mean=True, want_rgb=True):
    """The C call with sentinel-filled outputs; returns (rc, outputs untouched)."""
    rows, wt = film._shape
    mean, rgb = np.full((rows, wt, 3), -7.25), np.full((rows, wt, 3), 0xA5, np.uint8)
    st = GuidedStats(-1.0, -1.0, -1.0, -1.0)
    rc = film._lib.ykgpu_film_denoise_guided(film._f, ctypes.byref(dp) if dp is not None else None,
                                             ctypes.byref(fp) if fp is not None else None,
                                             mean.ctypes.data if want_mean else None,
                                             rgb.ctypes.data if want_rgb else None, ctypes.byref(st))
    untouched = bool((mean == -7.25).all() and (rgb == 0xA5).all() and st.total_ms == -1.0 and st.filter_ms == -1.0 and
                     st.features_ms == -1.0)
    return rc, untouched


def test_guided_errors_leave_the_outputs_untouched(ren):
    scene = refscenes.ref4()
    ren.set_scene(scene, CAM)
    p = make_params(**REF4_20)
    nan = float("nan")
    with ren.film(p) as film:
        assert raw_guided(film) == (YK_ERR_INVALID, True)  # fresh: count 0
        film.accumulate(1)
        assert raw_guided(film) == (YK_ERR_INVALID, True)  # one sample
        with pytest.raises(yk.YkError, match="YK_ERR_INVALID.*two samples"):
            film.denoise_guided()
        film.accumulate(3)
        for dp in (DenoiseParams(11, 1, 0.5, 1.0, 1e-10), DenoiseParams(5, 4, 0.5, 1.0, 1e-10),
                   DenoiseParams(5, 1, 0.0, 1.0, 1e-10), DenoiseParams(5, 1, 0.5, 1.0, 0.0),
                   DenoiseParams(5, 1, nan, 1.0, 1e-10), DenoiseParams(5, 1, 0.5, -1.0, 1e-10)):
            assert raw_guided(film, dp) == (YK_ERR_INVALID, True), dp.as_dict()
        for fp in (FeatureParams(0, 0, 1.0, 1.0, 1.0, 1.0, 1.0), FeatureParams(5, 0, 1.0, 1.0, 1.0, 1.0, 1.0),
                   FeatureParams(2, 1, 1.0, 1.0, 1.0, 1.0, 1.0), FeatureParams(2, 0, 0.0, 1.0, 1.0, 1.0, 1.0),
                   FeatureParams(2, 0, nan, 1.0, 1.0, 1.0, 1.0), FeatureParams(2, 0, INF, 1.0, 1.0, 1.0, 1.0),
                   FeatureParams(2, 0, 1.0, -1.0, 1.0, 1.0, 1.0), FeatureParams(2, 0, 1.0, nan, 1.0, 1.0, 1.0),
                   FeatureParams(2, 0, 1.0, 1.0, 0.0, 1.0, 1.0), FeatureParams(2, 0, 1.0, 1.0, 1.0, -1.0, 1.0),
                   FeatureParams(2, 0, 1.0, 1.0, 1.0, 1.0, nan)):
            assert raw_guided(film, None, fp) == (YK_ERR_INVALID, True), (fp.as_dict(), fp.reserved)
        assert raw_guided(film, want_mean=False, want_rgb=False) == (YK_ERR_INVALID, True)
        assert raw_guided(film) == (0, False)  # NULL params: the defaults
        S, Q = film_ref.prefixes(film_ref.colours(scene, CAM, p))
        check(film, scene, CAM, p, S[4], Q[4], 4, "after the refused calls")
        # one pixel below two samples in a non-uniform film: found on the device
        counts = np.full((9, 16), 4, np.uint32)
        counts[5, 7] = 1
        film.write_counts(far.at_counts(S, counts), far.at_counts(Q, counts), counts)
        assert raw_guided(film) == (YK_ERR_INVALID, True)
    # strided tiles have no neighbours to filter over (their features exist all the same)
    for kw in (dict(rows=(1, 4, 2)), dict(cols=(3, 5, 2)), dict(rows=(0, 4, 2, 1))):
        with ren.film(make_params(**REF4_20, **kw)) as film:
            film.accumulate(4)
            assert raw_guided(film) == (YK_ERR_UNSUPPORTED, True), kw
            with pytest.raises(yk.YkError, match="YK_ERR_UNSUPPORTED"):
                film.denoise_guided()
            film.features(2)


def test_one_shot_render_after_a_guided_denoise_equals_the_golden(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    with ren.film(make_params(**REF4_20)) as film:
        film.accumulate(4)
        film.denoise_guided(*params_of(dict(radius=10, patch=3)))
        got = ren.render(make_params(16, 9, 2, 50, 404))
        assert golden_data.sha(got) == golden_data.manifest()["constexpr_build"]["rgb_sha256"]
        film.denoise_guided()
    assert golden_data.sha(ren.render(make_params(16, 9, 2, 50, 404))) == \
        golden_data.manifest()["constexpr_build"]["rgb_sha256"]
