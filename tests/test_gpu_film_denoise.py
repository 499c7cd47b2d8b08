"""ykgpu_film_denoise on the MI355X (include/ykgpu.h "film denoise"): the filtered mean and its RGB8
image compared byte for byte, with no tolerance, with the numpy restatement of the definition
(film_denoise_ref) on the oracle's prefix folds; the film's state read back afterwards and asserted
unchanged.  The shapes are the smallest at which each path of the kernels is taken: a window that
crosses every edge, a halo larger than the image, sizes that are no multiple of the 32 x 8 block,
several blocks with interior halos, a sub-tile whose edge is not the image's, per-pixel counts, and
zero variance (the eps path).
"""
import ctypes

import numpy as np
import pytest

import film_adaptive_ref as far
import film_denoise_ref as fdr
import film_ref
import golden_data
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd.records import PRECISION_FP32, RNG_XOR128, DenoiseParams, make_params

pytestmark = pytest.mark.gpu

CAM = refscenes.reference_camera()
REF4_20 = dict(width=16, height=9, spp=20, max_depth=50, seed0=404)
YK_ERR_INVALID, YK_ERR_UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def ren():
    r = yk.Renderer(0)
    yield r
    r.close()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check(film, sums, sumsq, counts, what, **params):
    """One denoise against the yardstick on the state (sums, sumsq, counts) the film must hold."""
    before = film.read() + (film.counts(),)
    assert same(before[0], sums) and same(before[1], sumsq), f"the film's state {what}"
    mean, rgb, st = film.denoise(**params)
    want = fdr.denoise(sums, sumsq, counts, **params)
    assert same(mean, want), f"mean {what}: {int((mean != want).sum())} of {want.size} values differ"
    assert same(rgb, fdr.to_rgb8(want)), f"rgb {what}"
    assert st["moments_ms"] >= 0 and st["filter_ms"] > 0 and st["total_ms"] >= st["filter_ms"]
    after = film.read() + (film.counts(),)
    assert all(same(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(before, after)), f"state {what}"
    return mean, rgb


@pytest.mark.parametrize("params", [dict(), dict(radius=1, patch=0), dict(radius=10, patch=3)],
                         ids=["defaults", "r1-f0", "r10-f3"])
def test_ref4_after_chunks_of_4_and_16(ren, params):
    p = make_params(**REF4_20)
    ren.set_scene(refscenes.ref4(), CAM)
    S, Q = film_ref.prefixes(film_ref.colours(refscenes.ref4(), CAM, p))
    with ren.film(p) as film:
        film.accumulate(4)
        check(film, S[4], Q[4], 4, "after 4", **params)
        film.accumulate(16)
        mean, rgb = check(film, S[20], Q[20], 20, "after 20", **params)
        # either output alone
        only_mean, none, _ = film.denoise(want_rgb=False, **params)
        none2, only_rgb, _ = film.denoise(want_mean=False, **params)
        assert none is None and none2 is None and same(only_mean, mean) and same(only_rgb, rgb)
        assert film.accumulate_adaptive(-1.0, 1).pixels_selected == 0  # (complete, and still usable)


def test_radius_zero_is_the_mean(ren):
    p = make_params(**REF4_20)
    ren.set_scene(refscenes.ref4(), CAM)
    S, Q = film_ref.prefixes(film_ref.colours(refscenes.ref4(), CAM, p))
    with ren.film(p) as film:
        film.accumulate(4)
        for patch in (0, 3):
            mean, rgb = check(film, S[4], Q[4], 4, f"radius 0 patch {patch}", radius=0, patch=patch)
            assert same(mean, S[4] / 4.0) and same(rgb, film.resolve())


def test_sizes_that_are_no_multiple_of_a_block_and_a_sub_tile(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    p = make_params(37, 20, 8, 50, 404)
    S, Q = film_ref.prefixes(film_ref.colours(refscenes.ref4(), CAM, p))
    with ren.film(p) as film:
        film.accumulate(8)
        whole, _ = check(film, S[8], Q[8], 8, "37x20")
    # rows 3..14 and columns 5..30 of the same image: the tile's edge is the filter's edge
    sub = make_params(37, 20, 8, 50, 404, rows=(3, 12, 1), cols=(5, 26, 1))
    with ren.film(sub) as film:
        film.accumulate(8)
        s, q = np.ascontiguousarray(S[8][3:15, 5:31]), np.ascontiguousarray(Q[8][3:15, 5:31])
        part, _ = check(film, s, q, 8, "sub-tile")
    assert part.shape == (12, 26, 3) and not same(part, np.ascontiguousarray(whole[3:15, 5:31]))
    # consecutive rows named through bands (two bands of two rows, every band) are a tile like any other
    banded = make_params(37, 20, 8, 50, 404, rows=(2, 4, 1, 1))
    with ren.film(banded) as film:
        film.accumulate(8)
        check(film, np.ascontiguousarray(S[8][2:6]), np.ascontiguousarray(Q[8][2:6]), 8, "banded rows", radius=2)


def test_mixed12_several_blocks_and_it_denoises(ren):
    ren.set_scene(refscenes.mixed12(), CAM)
    p = make_params(64, 36, 16, 50, 404)
    S, Q = film_ref.prefixes(film_ref.colours(refscenes.mixed12(), CAM, p))
    with ren.film(p) as film:
        film.accumulate(16)
        mean, _ = check(film, S[16], Q[16], 16, "mixed12 64x36")
    truth = fdr.truth(refscenes.mixed12(), CAM, 64, 36)
    raw, filt = fdr.mse(S[16] / 16.0, truth), fdr.mse(mean, truth)
    print("mixed12 64x36x16: raw", repr(raw), "filtered", repr(filt), "ratio", filt / raw)
    assert filt <= 0.8 * raw


def adaptive(ren, p, zero_variance=False):
    ren.set_scene(refscenes.ref4(), CAM)
    sim = far.Sim(film_ref.colours(refscenes.ref4(), CAM, p))
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
            check(film, sim.sums(), sim.sumsq(), sim.counts, f"after pass {i}")
    assert any(lo != hi for lo, hi in spreads), spreads  # (a non-uniform film was filtered)


def test_non_uniform_film(ren):
    adaptive(ren, make_params(**REF4_20))


def test_zero_variance_pixels_fp32_xor128(ren):
    adaptive(ren, make_params(**REF4_20, precision=PRECISION_FP32, rng=RNG_XOR128), zero_variance=True)


def raw_denoise(film, dp=None, want_mean=True, want_rgb=True):
    """The C call with sentinel-filled outputs; returns (rc, outputs untouched)."""
    rows, wt = film._shape
    mean, rgb = np.full((rows, wt, 3), -7.25), np.full((rows, wt, 3), 0xA5, np.uint8)
    st = yk.DenoiseStats(-1.0, -1.0, -1.0)
    rc = film._lib.ykgpu_film_denoise(film._f, ctypes.byref(dp) if dp is not None else None,
                                      mean.ctypes.data if want_mean else None, rgb.ctypes.data if want_rgb else None,
                                      ctypes.byref(st))
    untouched = bool((mean == -7.25).all() and (rgb == 0xA5).all() and st.total_ms == -1.0 and st.filter_ms == -1.0)
    return rc, untouched


def test_errors_leave_the_outputs_untouched(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    p = make_params(**REF4_20)
    with ren.film(p) as film:
        assert raw_denoise(film) == (YK_ERR_INVALID, True)  # fresh: count 0
        film.accumulate(1)
        assert raw_denoise(film) == (YK_ERR_INVALID, True)  # one sample
        with pytest.raises(yk.YkError, match="YK_ERR_INVALID.*two samples"):
            film.denoise()
        film.accumulate(3)
        bad = [DenoiseParams(11, 1, 0.5, 1.0, 1e-10), DenoiseParams(5, 4, 0.5, 1.0, 1e-10),
               DenoiseParams(5, 1, 0.0, 1.0, 1e-10), DenoiseParams(5, 1, 0.5, 1.0, 0.0),
               DenoiseParams(5, 1, float("nan"), 1.0, 1e-10), DenoiseParams(5, 1, 0.5, float("nan"), 1e-10),
               DenoiseParams(5, 1, 0.5, 1.0, float("nan")), DenoiseParams(5, 1, float("inf"), 1.0, 1e-10),
               DenoiseParams(5, 1, 0.5, -1.0, 1e-10)]
        for dp in bad:
            assert raw_denoise(film, dp) == (YK_ERR_INVALID, True), dp.as_dict()
        assert raw_denoise(film, want_mean=False, want_rgb=False) == (YK_ERR_INVALID, True)
        assert raw_denoise(film, None) == (0, False)  # NULL params: the defaults
        S, Q = film_ref.prefixes(film_ref.colours(refscenes.ref4(), CAM, p))
        check(film, S[4], Q[4], 4, "after the refused calls")
        # one pixel below two samples in a non-uniform film: found on the device
        counts = np.full((9, 16), 4, np.uint32)
        counts[5, 7] = 1
        film.write_counts(far.at_counts(S, counts), far.at_counts(Q, counts), counts)
        assert raw_denoise(film) == (YK_ERR_INVALID, True)
    # strided tiles have no neighbours to filter over
    for kw in (dict(rows=(1, 4, 2)), dict(cols=(3, 5, 2)), dict(rows=(0, 4, 2, 1))):
        with ren.film(make_params(**REF4_20, **kw)) as film:
            film.accumulate(4)
            assert raw_denoise(film) == (YK_ERR_UNSUPPORTED, True), kw
            with pytest.raises(yk.YkError, match="YK_ERR_UNSUPPORTED"):
                film.denoise()


def test_one_shot_render_after_a_denoise_equals_the_golden(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    with ren.film(make_params(**REF4_20)) as film:
        film.accumulate(4)
        film.denoise(radius=10, patch=3)
        got = ren.render(make_params(16, 9, 2, 50, 404))
        assert golden_data.sha(got) == golden_data.manifest()["constexpr_build"]["rgb_sha256"]
        film.denoise()
    assert golden_data.sha(ren.render(make_params(16, 9, 2, 50, 404))) == \
        golden_data.manifest()["constexpr_build"]["rgb_sha256"]
